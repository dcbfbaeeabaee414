"""cycle_scenes.py -- the graphs of tests/test_cycle.py and tests/test_cycle_cpp.py (test infrastructure, NOT product code).

Every scene is a dict n_views, src, dst (int64 [P]), R [P,3,3] (R_dst_src), t [P,3] (unit t_dst_src), status [P] (int32) and,
where it has one, the ground truth R_gt [V,3,3] (world->camera), c_gt [V,3] and bad [P] (the records replaced by a random
pose).  An edge (s, d) of the ground truth: R = R_d R_s^T, t = R_d (c_s - c_d) / |.| (x_d = R x_s + t up to the baseline's
length).  Seeds are fixed; a seed whose scene fails test_margin_condition is replaced, the condition stays.
"""
import functools

import numpy as np

import cycle_spec as CS


def random_rotation(rng, max_deg=180.0):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = np.radians(rng.uniform(0.0, max_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def small_rotation(rng, deg):
    """A rotation by exactly deg degrees about a random axis."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def random_poses(rng, n, spread=4.0):
    return np.stack([random_rotation(rng) for _ in range(n)]), rng.uniform(-spread, spread, (n, 3))


def relative(R_gt, c_gt, s, d):
    R = R_gt[d] @ R_gt[s].T
    t = R_gt[d] @ (c_gt[s] - c_gt[d])
    return R, t / np.linalg.norm(t)


def invert(R, t):
    return R.T.copy(), -(R.T @ t)


def from_pairs(R_gt, c_gt, pairs, status=None, bad=None):
    P = len(pairs)
    R, t = np.zeros((P, 3, 3)), np.zeros((P, 3))
    for p, (s, d) in enumerate(pairs):
        R[p], t[p] = relative(R_gt, c_gt, s, d)
    pr = np.array(pairs, np.int64).reshape(P, 2)
    return dict(n_views=len(R_gt), src=pr[:, 0].copy(), dst=pr[:, 1].copy(), R=R, t=t,
                status=np.full(P, CS.EDGE_OK, np.int32) if status is None else np.asarray(status, np.int32),
                R_gt=R_gt, c_gt=c_gt, bad=np.zeros(P, bool) if bad is None else bad)


def corrupt(scene, which, rng):
    """Replaces the records `which` by random poses (in place); marks them in scene['bad']."""
    for p in which:
        scene["R"][p] = random_rotation(rng)
        v = rng.standard_normal(3)
        scene["t"][p] = v / np.linalg.norm(v)
        scene["bad"][p] = True
    return scene


def flip(scene, which):
    """Stores the records `which` the other way round: (dst, src) with the inverted pose (in place)."""
    for p in which:
        scene["src"][p], scene["dst"][p] = scene["dst"][p], scene["src"][p]
        scene["R"][p], scene["t"][p] = invert(scene["R"][p], scene["t"][p])
    return scene


# ---- the scenes -----------------------------------------------------------------------------------------------------------
TRIANGLE_SEED = 11


def triangle(pattern=0, seed=TRIANGLE_SEED):
    """Three views in general position, pairs (0,1), (1,2), (0,2); bit k of pattern stores pair k flipped."""
    rng = np.random.default_rng(seed)
    R_gt, c_gt = random_poses(rng, 3)
    sc = from_pairs(R_gt, c_gt, [(0, 1), (1, 2), (0, 2)])
    return flip(sc, [k for k in range(3) if pattern >> k & 1])


def collinear_triangle(seed=TRIANGLE_SEED):
    rng = np.random.default_rng(seed)
    R_gt, _ = random_poses(rng, 3)
    d = np.array([0.6, -0.3, 0.74])
    c_gt = np.stack([0.0 * d, 1.0 * d, 2.5 * d])
    return from_pairs(R_gt, c_gt, [(0, 1), (1, 2), (0, 2)])


def k4(seed=12):
    """K4 with the record (0, 1) replaced by a random pose: its two triangles are bad, every other edge keeps one good one."""
    rng = np.random.default_rng(seed)
    R_gt, c_gt = random_poses(rng, 4)
    sc = from_pairs(R_gt, c_gt, [(0, 1), (0, 2), (3, 0), (1, 2), (3, 1), (2, 3)])
    return corrupt(sc, [0], rng)


def bridge(seed=13):
    """A triangle (0, 1, 2) and the bridge (2, 3), which lies in no triangle."""
    rng = np.random.default_rng(seed)
    R_gt, c_gt = random_poses(rng, 4)
    return from_pairs(R_gt, c_gt, [(0, 1), (2, 1), (0, 2), (2, 3)])


def random_graph(seed=14, V=40, E=200, non_ok=0.2, bad=0.1, noise_deg=0.5):
    """V views, E distinct random pairs in random orientation, a share non_ok of them with a failure status (and a random
    pose), a share bad of the rest replaced by random poses, small noise on the others."""
    rng = np.random.default_rng(seed)
    R_gt, c_gt = random_poses(rng, V)
    allp = [(a, b) for a in range(V) for b in range(a + 1, V)]
    pairs = [allp[i] for i in rng.choice(len(allp), E, replace=False)]
    pairs = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pairs]
    status = np.where(rng.random(E) < non_ok, rng.choice([0, -1, -2, -3], E), CS.EDGE_OK).astype(np.int32)
    sc = from_pairs(R_gt, c_gt, pairs, status)
    for p in range(E):
        sc["R"][p] = small_rotation(rng, noise_deg * rng.random()) @ sc["R"][p]
    ok = np.nonzero(status == CS.EDGE_OK)[0]
    corrupt(sc, np.concatenate([rng.choice(ok, int(bad * len(ok)), replace=False), np.nonzero(status != CS.EDGE_OK)[0]]), rng)
    return sc


WHEEL_RIM = 300


def wheel(seed=15, rim=WHEEL_RIM):
    """A hub of degree `rim` whose id lies in the middle of the rim's consecutive ids (rim ids 0 .. rim/2 - 1 and
    rim/2 + 1 .. rim; the hub is rim/2), so that the pairs (a, hub) cut the hub's list at every place and the pairs
    (hub, b) cut the rim lists above the hub.  Rim views are joined to their successors (a cycle); the spokes alternate in
    orientation and every tenth is replaced by a random pose."""
    rng = np.random.default_rng(seed)
    V = rim + 1
    hub = rim // 2
    R_gt, c_gt = random_poses(rng, V)
    ring = [v for v in range(V) if v != hub]
    ang = 2 * np.pi * np.arange(rim) / rim
    c_gt[ring] = np.stack([10 * np.cos(ang), 10 * np.sin(ang), rng.uniform(-2, 2, rim)], 1)
    c_gt[hub] = np.array([1.0, -2.0, 6.0])
    spokes = [(hub, v) if k % 2 else (v, hub) for k, v in enumerate(ring)]
    rims = [(ring[k], ring[(k + 1) % rim]) for k in range(rim)]
    sc = from_pairs(R_gt, c_gt, spokes + rims)
    return corrupt(sc, list(range(0, rim, 10)), rng)


def no_ok_records(seed=16):
    rng = np.random.default_rng(seed)
    R_gt, c_gt = random_poses(rng, 5)
    return from_pairs(R_gt, c_gt, [(0, 1), (1, 2), (0, 2), (3, 4)], status=[0, -1, -2, 0])


def empty():
    z = np.zeros(0, np.int64)
    return dict(n_views=4, src=z, dst=z.copy(), R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)), status=np.zeros(0, np.int32),
                bad=np.zeros(0, bool))


VALUE_SEED = 21


@functools.lru_cache(maxsize=None)
def value_scene(seed=VALUE_SEED, V=60, chords=240, max_span=6, r_noise_deg=0.3, t_noise_deg=1.0, bad=0.15):
    """The ground-truth graph of the value test: a ring over V views plus random chords (300 edges), noise on every R and
    t, a share bad of the edges replaced by random poses.  The chords are drawn among the view pairs 2 .. max_span apart on
    the ring, as in a sequence-like capture: chords drawn among ALL view pairs leave most edges of a 300-edge graph in a
    single triangle, and then 7 to 14 % of the true edges lose their only triangle to a corrupted neighbour (measured on
    ten seeds) -- no seed comes near the 2 % cap of the value test there."""
    rng = np.random.default_rng(seed)
    R_gt, c_gt = random_poses(rng, V)
    ring = [(v, (v + 1) % V) for v in range(V)]
    rest = [(v, (v + k) % V) for v in range(V) for k in range(2, max_span + 1)]
    pairs = ring + [rest[i] for i in rng.choice(len(rest), chords, replace=False)]
    sc = from_pairs(R_gt, c_gt, pairs)
    for p in range(len(pairs)):
        sc["R"][p] = small_rotation(rng, r_noise_deg) @ sc["R"][p]
        sc["t"][p] = small_rotation(rng, t_noise_deg) @ sc["t"][p]
    corrupt(sc, rng.choice(len(pairs), int(bad * len(pairs)), replace=False), rng)
    for k in ("src", "dst", "R", "t", "status", "bad"):
        sc[k].setflags(write=False)
    return sc


def run_spec(sc, **params):
    return CS.cycle_filter(sc["n_views"], sc["src"], sc["dst"], sc["R"], sc["t"], sc["status"], details=True, **params)


def edge_table(sc, rng=None):
    """The scene as pgi_edge records (numpy structured, pyposegraphbuilder.EDGE_DTYPE): R, t, status from the scene, the
    other fields filled with arbitrary values so that a copy that loses a byte shows."""
    from pyposegraphbuilder import EDGE_DTYPE
    rng = np.random.default_rng(5) if rng is None else rng
    P = len(sc["src"])
    raw = rng.integers(0, 256, (P, EDGE_DTYPE.itemsize), dtype=np.uint8)
    e = raw.view(EDGE_DTYPE).reshape(P).copy()
    e["E"] = rng.standard_normal((P, 9))
    e["R"], e["t"], e["status"] = sc["R"].reshape(P, 9), sc["t"], sc["status"]
    return e


def gpu_scenes():
    """name -> scene: every graph the GPU tests run (test_margin_condition checks each)."""
    out = {"triangle_%d" % k: triangle(k) for k in range(8)}
    out.update(k4=k4(), bridge=bridge(), random=random_graph(), wheel=wheel(), no_ok=no_ok_records(), empty=empty(),
               value=value_scene())
    return out
