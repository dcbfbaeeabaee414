#!/usr/bin/env python3
"""Turns the rocprofv3 PMC summaries of scripts/profile_k1.sh <tag> (gpurun_out/<tag>_k1_*_summary.txt) into
profiles/<tag>_k1_pmc.json (usage: k1_pmc_json.py r03 [git head]): HBM traffic (with the gfx950 FETCH_SIZE correction), the wave-lifetime split, and the
EXECUTED floating-point work per launch for an honest compute roofline next to the (nominated) HBM one.

flop counting: SQ_INSTS_VALU_{ADD,MUL,TRANS}_Fxx count wave-instructions (1 flop per lane), SQ_INSTS_VALU_FMA_Fxx 2 flop
per lane; 64 lanes per wave-instruction are charged although EXEC masks part of them (the solver keeps 10-16 of every
16 lanes busy), so the figure is an UPPER bound on useful flop and exact for issue-slot occupancy."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gpurun_out")
PEAK_F32, PEAK_F64 = 157.3e12, 78.6e12


TAG = sys.argv[1] if len(sys.argv) > 1 else "r04"


def read(tag, kernel="estimate_pose_kernel<2, false, 4>"):
    vals, avg_us, calls = {}, None, None
    for line in open(os.path.join(OUT, "%s_k1_%s_summary.txt" % (TAG, tag))):
        if kernel not in line:
            continue
        m = re.search(r"(\S+)\s+n=(\d+)\s+sum=(\S+)", line)
        if m:
            vals[m.group(1)] = (float(m.group(3)), int(m.group(2)))
        else:
            f = line.split(")")[-1].split()
            calls, avg_us = int(f[0]), float(f[2])
    return vals, avg_us, calls


def unprofiled_kernel_us():
    try:
        line = [ln for ln in open(os.path.join(OUT, "%s_k1_unprofiled_bench.json" % TAG)) if ln.startswith("{")][-1]
        return round(1e3 * json.loads(line)["roofline"]["kernel_ms"], 1)
    except Exception:  # noqa: BLE001
        return None


def main():
    trace, avg_us, calls = read("trace")
    c = {}
    for tag in ("flops", "mix", "wait", "lds", "fetch", "write"):
        v, a, n = read(tag)
        for k, (s, cnt) in v.items():
            c[k] = s / cnt          # per launch
        c["_avg_us_" + tag] = a
    flop32 = 64 * (c["SQ_INSTS_VALU_ADD_F32"] + c["SQ_INSTS_VALU_MUL_F32"] + c["SQ_INSTS_VALU_TRANS_F32"] + 2 * c["SQ_INSTS_VALU_FMA_F32"])
    flop64 = 64 * (c["SQ_INSTS_VALU_ADD_F64"] + c["SQ_INSTS_VALU_MUL_F64"] + c["SQ_INSTS_VALU_TRANS_F64"] + 2 * c["SQ_INSTS_VALU_FMA_F64"])
    sec = avg_us * 1e-6
    fetch_b = c["FETCH_SIZE"] * 1024 * 2      # gfx950: FETCH_SIZE tallies 64 B per 128-B request (MI355X_MICROARCH.md, HBM)
    write_b = c["WRITE_SIZE"] * 1024
    wc = c["SQ_WAVE_CYCLES"]
    out = {
        "kernel": "pgi::estimate_pose_kernel<2, false, 4> (hybrid rows: 1280 in LDS, 720 from L2; four wavefronts per pair at this batch size)", "pairs": 10000, "corrs": 2000,
        "profile_tag": TAG,
        "source": "rocprofv3 --kernel-trace --pmc ... (separate passes, scripts/profile_k1.sh %s); sums / dispatches; "
                  "summaries in profiles/%s_k1_rocprofv3_summary.txt" % (TAG, TAG),
        # ties these counters to the kernels that were timed: bench.py replays them only while this hash equals the hash
        # of the sources it runs (pyposegraphbuilder._lib.kernel_source_sha256: csrc/pgi_kernels.hip + pgi_device.hpp + pgi_normal_monomials.hpp)
        "source_sha256": open(os.path.join(OUT, "%s_k1_source_sha256.txt" % TAG)).read().strip(),
        "git_head": sys.argv[2] if len(sys.argv) > 2 else None,
        "kernel_us_trace_avg": avg_us, "dispatches": calls,
        # the same bench command without the profiler on the same lease (HIP events on the launch stream): what the profiled
        # average is to be reconciled with -- the profiler adds a few per cent
        "kernel_us_events_same_box": unprofiled_kernel_us(),
        "launch_shape": "size-class launches are persistent grids (256 CUs x 4 resident workgroups pull pairs from the class's list "
                        "through an atomic head).  An EMPTY class still shows milliseconds in the kernel trace (estimate_pose_kernel<1, false> "
                        "on this workload): its workgroups are queued on a side stream behind the other class's resident workgroups, which "
                        "hold every LDS slot until their list runs dry -- the time is waiting for a slot, each workgroup exits at once "
                        "when it gets one",
        "hbm_bytes_per_launch": round(fetch_b + write_b), "fetch_size_kb_per_launch": round(c["FETCH_SIZE"]),
        "write_size_kb_per_launch": round(c["WRITE_SIZE"]),
        "correction": "FETCH_SIZE x2 on gfx950 (64 B tallied per 128-B request); WRITE_SIZE as reported",
        "algorithmic_bytes_per_launch": 10000 * (17 * 2000 + 200),
        "executed_flop_per_launch": {"f32": round(flop32), "f64": round(flop64),
                                     "note": "wave-instructions x 64 lanes (EXEC masks not subtracted): upper bound on useful flop"},
        "roofline_compute": {
            "f32_tflops": round(flop32 / sec / 1e12, 2), "f32_frac_of_157.3": round(flop32 / sec / PEAK_F32, 4),
            "f64_tflops": round(flop64 / sec / 1e12, 2), "f64_frac_of_78.6": round(flop64 / sec / PEAK_F64, 4),
            "valu_time_frac": round(flop32 / sec / PEAK_F32 + flop64 / sec / PEAK_F64, 4),
            "note": "valu_time_frac = share of the chip's VALU issue time the executed FP instructions need at peak rate "
                    "(f32 and f64 share the pipes); integer / move / compare / DPP instructions are extra"},
        "valu_instruction_mix_per_launch": {k: round(c[k]) for k in sorted(c) if k.startswith("SQ_INSTS_")},
        "mfma_instructions": round(c.get("SQ_INSTS_MFMA", 0)),
        "wave_lifetime_split": {"waiting_on_waitcnt_or_barrier": round(c["SQ_WAIT_ANY"] / wc, 3),
                                "issue_stalled": round(c["SQ_WAIT_INST_ANY"] / wc, 3),
                                "issuing": round(c["SQ_ACTIVE_INST_ANY"] / wc, 3)},
        "lds_bank_conflict_frac_of_lds_active": round(c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"], 4),
        "thread_cycles_valu_per_valu_instruction": round(c["SQ_THREAD_CYCLES_VALU"] / c["SQ_INSTS_VALU"], 2),
        "grbm_gui_active_per_launch": round(c["GRBM_GUI_ACTIVE"]),
        "shader_clock_ghz_est": round(c["GRBM_GUI_ACTIVE"] / 8 / (c["_avg_us_lds"] * 1e-6) / 1e9, 3),  # summed over the 8 XCDs
    }
    # SIMD-level view: a wave64 VALU instruction holds its SIMD's vector ALU for 4 cycles (16 lanes per cycle; f64 FMA and
    # unpacked f32 alike -- the 157.3 TFLOP/s f32 peak assumes v_pk_* instructions); transcendental, f64 division / sqrt
    # sequences and 32-bit integer multiplies take longer, so this is a LOWER bound on how busy the vector ALUs are.
    simd_cycles = c["GRBM_GUI_ACTIVE"] / 8 * (c["_avg_us_mix"] / c["_avg_us_lds"]) * 1024
    out["valu_issue_busy_frac"] = round(c["SQ_INSTS_VALU"] * 4 / simd_cycles, 3)
    out["roofline_compute"]["valu_issue_busy_frac"] = out["valu_issue_busy_frac"]  # travels with bench.py's roofline_compute
    out["roofline_compute"]["note"] += ("; valu_issue_busy_frac = SQ_INSTS_VALU x 4 cycles / SIMD cycles, a lower bound on vector-ALU "
                                        "occupancy (the kernel is issue-bound); v_pk_* instructions count once, so f32_tflops "
                                        "understates the packed scoring arithmetic")
    out["valu_issue_busy_note"] = ("SQ_INSTS_VALU x 4 cycles / (shader cycles x 1024 SIMDs): the kernel is bound by vector-ALU issue, "
                                   "not by memory or latency -- the per-wave 'waiting' share is time spent behind the other three "
                                   "wavefronts of the SIMD")
    dst = os.path.join(ROOT, "profiles", "%s_k1_pmc.json" % TAG)
    json.dump(out, open(dst, "w"), indent=2)
    print(json.dumps(out, indent=2))


if __name__ == "__main__":
    main()
