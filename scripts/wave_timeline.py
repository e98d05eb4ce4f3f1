#!/usr/bin/env python
"""Wave time line of the headline kernel (k_bdf_adaptive<.., FAST, WAVE, DEFOPT>, the instantiation bench.py times): where every wavefront of a launch ran, when it
started and ended, and what it cost.  A DIAGNOSTIC build: the library compiled with -DDSH_WAVE_TIMELINE=1 (dsh_adaptive_kernel.hpp) into a directory of its own,
loaded through DSH_LIB_DIR; lane 0 of every wavefront stores (s_memrealtime at entry and after the last step, HW_ID, XCC_ID, blockIdx.x, its step and Newton counters)
to a buffer of the library's.  The stamps cost two stores per wavefront and nothing inside the step loop; quote this build's SHARES, not its length.

    python scripts/wave_timeline.py build [--tag T] [-D NAME=VALUE ...]     no GPU: make -C diffsol_amd/csrc OUT=../lib_exp/timeline_T with the switch and the defines
    python scripts/wave_timeline.py run   [--tag T] [--sizes 65536 100000] [--solves 3]     GPU: markdown on stdout

`-D DSH_PAIR_PRIO=0` gives the time line of the kernel without the priority policy.  Per ensemble size, from the last of the recorded solves (the others give the
spread of the launch's span):
  1. how many SIMDs hold 0, 1, 2 or more wavefronts, wavefronts per CU;
  2. finish time (from the launch's first stamp) and wavefront life per Newton iteration of the group, for singly occupied SIMDs and for the first and the
     second arrival of doubly occupied ones;
  3. whether the second arrival is the wavefront with blockIdx.x >= 4 * CUs, and which hardware wave slot the arrivals sit in."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = [("t_in", "<u8"), ("t_out", "<u8"), ("block", "<u4"), ("hw_id", "<u4"), ("xcc_id", "<u4"), ("n_steps", "<u4"), ("n_newton", "<u4"), ("pad", "<u4")]  # WaveTimelineRecord
TICK_US = 0.01  # s_memrealtime: 100 MHz


def lib_dir(tag):
    return os.path.join(ROOT, "diffsol_amd", "lib_exp", "timeline" + ("_" + tag if tag else ""))


def build(tag, defines):
    import re
    mk = open(os.path.join(ROOT, "diffsol_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950")
    flags += " -DDSH_WAVE_TIMELINE=1" + "".join(f" -D{d}" for d in defines)
    out = lib_dir(tag)
    subprocess.run(["make", "-C", os.path.join(ROOT, "diffsol_amd", "csrc"), f"-j{min(8, len(os.sched_getaffinity(0)))}", f"OUT={out}", f"HIPFLAGS={flags}"], check=True)
    host = os.path.join(ROOT, "diffsol_amd", "lib", "libdiffsol_hip_host.so")  # DSH_LIB_DIR holds both libraries; the host one has no switch
    if not os.path.exists(host):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diffsol_amd", "host")], check=True)
    subprocess.run(["cp", host, out], check=True)
    print(out)


def pct(a, q):
    import numpy as np
    return float(np.percentile(a, q)) if len(a) else float("nan")


def row(name, a, fmt):
    import numpy as np
    a = np.asarray(a, dtype=float)
    if not len(a):
        return f"| {name} | 0 | | | | | |"
    return f"| {name} | {len(a)} | {fmt % a.min()} | {fmt % pct(a, 10)} | {fmt % pct(a, 50)} | {fmt % pct(a, 90)} | {fmt % a.max()} |"


def analyse(r, simds_total):
    """r: the records of one launch.  Prints the three items."""
    import numpy as np
    hw = r["hw_id"]
    slot, simd, cu, sh, se, xcc = hw & 0xF, (hw >> 4) & 3, (hw >> 8) & 0xF, (hw >> 12) & 1, (hw >> 13) & 7, r["xcc_id"] & 0xF
    cu_key = ((xcc.astype(np.int64) * 8 + se) * 2 + sh) * 16 + cu
    simd_key = cu_key * 4 + simd
    t0 = int(r["t_in"].min())
    start = (r["t_in"].astype(np.int64) - t0) * TICK_US
    finish = (r["t_out"].astype(np.int64) - t0) * TICK_US
    life = (r["t_out"].astype(np.int64) - r["t_in"].astype(np.int64)) * TICK_US
    per_newton = 1e3 * life / np.maximum(r["n_newton"], 1)  # ns of wavefront life per Newton iteration of the group
    keys, inv, cnt = np.unique(simd_key, return_inverse=True, return_counts=True)
    cus, cu_cnt = np.unique(cu_key, return_counts=True)
    print(f"{len(r)} wavefronts, launch span (first entry stamp to last exit stamp) {finish.max():.1f} us; {len(cus)} CUs and {len(keys)} SIMDs seen of {simds_total // 4} and {simds_total}.\n")
    print("| wavefronts on the SIMD | 0 | 1 | 2 | 3 | 4 or more |\n|---|---|---|---|---|---|")
    print(f"| SIMDs | {simds_total - len(keys)} | {(cnt == 1).sum()} | {(cnt == 2).sum()} | {(cnt == 3).sum()} | {(cnt >= 4).sum()} |\n")
    print("| wavefronts on the CU | " + " | ".join(str(k) for k in sorted(set(cu_cnt.tolist()))) + " |\n|---|" + "---|" * len(set(cu_cnt.tolist())))
    print("| CUs | " + " | ".join(str(int((cu_cnt == k).sum())) for k in sorted(set(cu_cnt.tolist()))) + f" |   ({simds_total // 4 - len(cus)} CUs hold none)\n")
    on = cnt[inv]
    single = on == 1
    order = np.lexsort((r["t_in"], simd_key))  # by SIMD, then by arrival
    rank = np.empty(len(r), dtype=np.int64)
    pos = np.arange(len(r))
    first_of = np.r_[0, np.nonzero(np.diff(simd_key[order]))[0] + 1]
    rank[order] = pos - np.repeat(first_of, np.diff(np.r_[first_of, len(r)]))
    first, second = (on == 2) & (rank == 0), (on == 2) & (rank == 1)
    # do the two of a SIMD overlap at all?  (a second wavefront that starts after the first ended is a later round, not a partner)
    a, b = order[np.nonzero(first[order])[0]], order[np.nonzero(second[order])[0]]
    if len(a):
        assert np.array_equal(simd_key[a], simd_key[b])
        overlap = r["t_in"][b] < r["t_out"][a]
        print(f"Doubly occupied SIMDs: {len(a)}; the second arrival starts before the first ends on {int(overlap.sum())} of them; "
              f"the second ends after the first on {int((r['t_out'][b] > r['t_out'][a]).sum())}.\n")
    print("| us / ns | wavefronts | min | p10 | median | p90 | max |\n|---|---|---|---|---|---|---|")
    for name, m in (("alone on its SIMD", single), ("first arrival of two", first), ("second arrival of two", second), ("on a SIMD with three or more", on >= 3)):
        if not m.any():
            continue
        print(row(f"{name}: entry stamp, us after the first", start[m], "%.1f"))
        print(row(f"{name}: finish, us", finish[m], "%.1f"))
        print(row(f"{name}: life, us", life[m], "%.1f"))
        print(row(f"{name}: Newton iterations of the group", r["n_newton"][m], "%.0f"))
        print(row(f"{name}: life per Newton iteration, ns", per_newton[m], "%.1f"))
    print()
    if len(a):
        ra, rb = per_newton[a], per_newton[b]
        print(f"Pairs: life per Newton iteration, second over first arrival: median {np.median(rb / ra):.3f} (p10 {pct(rb / ra, 10):.3f}, p90 {pct(rb / ra, 90):.3f}); "
              f"first arrival over the median of the wavefronts alone: {np.median(ra) / np.median(per_newton[single]) if single.any() else float('nan'):.3f}, "
              f"second: {np.median(rb) / np.median(per_newton[single]) if single.any() else float('nan'):.3f}.\n")
        late = r["block"] >= simds_total
        print(f"Second arrivals with blockIdx.x >= {simds_total}: {int(late[b].sum())} of {len(b)}; first arrivals with blockIdx.x >= {simds_total}: {int(late[a].sum())} of {len(a)}; "
              f"wavefronts alone: {int(late[single].sum())} of {int(single.sum())}.  Wavefronts with blockIdx.x >= {simds_total} in the launch: {int(late.sum())}.")
        sl = lambda m: ", ".join(f"slot {k}: {int((slot[m] == k).sum())}" for k in sorted(set(slot[m].tolist())))
        print(f"Hardware wave slot (HW_ID[3:0]): first arrivals {sl(a)}; second arrivals {sl(b)}; alone {sl(np.nonzero(single)[0])}.\n")


def run(tag, sizes, solves):
    os.environ["DSH_LIB_DIR"] = lib_dir(tag)
    assert os.path.exists(os.path.join(lib_dir(tag), "libdiffsol_hip.so")), f"no diagnostic build in {lib_dir(tag)}: python scripts/wave_timeline.py build --tag {tag}"
    sys.path.insert(0, ROOT)
    import numpy as np
    import diffsol_amd as H
    from diffsol_amd import _ffi
    from bench import robertson_params, T_EVAL, RTOL, ATOL
    import torch
    simds_total = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    dev = _ffi.load_device_lib()
    read = dev.dsh_wave_timeline_read  # exported by the diagnostic build only
    read.restype, read.argtypes = C.c_int64, [C.c_void_p, C.c_int64]
    for nb in sizes:
        p = robertson_params(max(nb, 100000))[:nb]
        s = H.Solver("robertson_ode", p, nbatch=nb, model_size=1, rtol=RTOL, atol=ATOL, block_threads=256)
        for _ in range(3):
            s.solve_dense(T_EVAL, want_host=False)
        spans, r = [], None
        for _ in range(solves):
            s.solve_dense(T_EVAL, want_host=False)
            buf = np.zeros((nb + 63) // 64, dtype=REC)
            n = read(buf.ctypes.data_as(C.c_void_p), len(buf))
            assert n == len(buf), (n, len(buf))
            r = buf
            assert np.array_equal(np.sort(r["block"]), np.arange(len(r))) and (r["t_out"] > r["t_in"]).all(), "the records are not one per wavefront of this launch"
            spans.append((int(r["t_out"].max()) - int(r["t_in"].min())) * TICK_US)
        print(f"### {nb} members" + (f" ({tag})" if tag else "") + "\n")
        print(f"Launch spans of {solves} recorded solves after 3: " + ", ".join(f"{v:.1f}" for v in spans) + " us.  The last one:\n")
        analyse(r, simds_total)
        sys.stdout.flush()
        del s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["build", "run"])
    ap.add_argument("--tag", default="")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 100000])
    ap.add_argument("--solves", type=int, default=3)
    a = ap.parse_args()
    if a.what == "build":
        build(a.tag, a.defines)
    else:
        run(a.tag, a.sizes, a.solves)
