#!/usr/bin/env python
"""BASELINE config 2 through the pure 1:1 trait composition (fused = False, lock-step): wall clock, for rocprofv3 --kernel-trace --stats

    python scripts/trait_path_once.py                 # three solves, immediate launches (as before)
    python scripts/trait_path_once.py --op-queue      # the same with the op queue on (dsh_ctx_set_op_queue): for the kernel trace of the queued path
    python scripts/trait_path_once.py --op-queue --alternate 6   # ONE process, after warm-up: off / on / off / on ..., 6 solves each, ms per solve and the queue's counters
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import diffsol_amd as H  # noqa: E402
from diffsol_amd.solver import ENSEMBLE_LOCKSTEP  # noqa: E402
from bench import robertson_params, T_EVAL, RTOL, ATOL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--op-queue", action="store_true", help="run with the op queue on")
ap.add_argument("--alternate", type=int, default=0, metavar="N", help="alternate queue off / on for N timed solves each in this process (implies --op-queue for the 'on' half)")
ap.add_argument("--nbatch", type=int, default=100000)
ap.add_argument("--solves", type=int, default=3)
ap.add_argument("--json", default=None, help="also write the figures to this file")
args = ap.parse_args()

nb = args.nbatch
s = H.Solver("robertson_ode", robertson_params(nb), nbatch=nb, model_size=1, rtol=RTOL, atol=ATOL, fused=False, ensemble_mode=ENSEMBLE_LOCKSTEP)


def one_solve(on):
    s.set_op_queue(on)
    s.reset()
    s.set_op_queue(on)  # again: resets the queue's counters, so that they are those of the solve alone
    t0 = time.perf_counter()
    s.solve_dense(T_EVAL, want_host=False)
    return time.perf_counter() - t0


if args.alternate:
    for on in (False, True, False, True):  # warm-up: both modes, twice
        one_solve(on)
    w = {False: [], True: []}
    q = st = None
    for _ in range(args.alternate):
        for on in (False, True):
            w[on].append(one_solve(on))
            if on:
                q, st = s.op_queue_stats(), s.stats()
    res = {}
    for on in (False, True):
        ms = [round(1e3 * x, 3) for x in w[on]]
        res["on" if on else "off"] = dict(ms=ms, min=min(ms), median=float(np.median(ms)), max=max(ms))
        print("trait path, op queue", "on: " if on else "off:", "ms per solve", ms, "min / median / max", min(ms), float(np.median(ms)), max(ms))
    res["op_queue_stats"], res["stats"] = q, st
    print("op queue counters of one solve:", q)
    print("ops per chain: %.2f" % (q["ops_enqueued"] / max(1, q["chain_launches"])), " launches saved per solve:", q["ops_enqueued"] - q["chain_launches"])
    print("stats:", st)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
else:
    s.set_op_queue(args.op_queue)
    s.solve_dense(T_EVAL, want_host=False)
    w = []
    for _ in range(args.solves):
        s.reset(); t0 = time.perf_counter(); s.solve_dense(T_EVAL, want_host=False); w.append(time.perf_counter() - t0)
    print("trait path%s: ms per solve" % (" (op queue on)" if args.op_queue else ""), [round(1e3 * x, 2) for x in w], s.stats())
    if args.op_queue:
        print("op queue counters since it was switched on:", s.op_queue_stats())
