#!/usr/bin/env python3
"""Rate of Engine.pose_graph_optimize (multiway registration, csrc/alignnet_posegraph.hip) on the restatement's synthetic tracks: whole calls
(host checks, uploads, one launch per chunk, downloads), median of 5 with min .. max, and the kernel's own time from the "pose_graph" timer.

    python tools/pose_graph_rate.py [--out profiles/pose_graph_rate.json]

Inputs, z-constrained form, three planted wrong edges per graph (tests/pose_graph_ref.track): 256 graphs of 12 nodes with window 4, 256 graphs of 100
nodes with window 4, 64 graphs of 25 nodes fully connected.  Recorded per input: which placement its bands took (LDS or workspace), solves, and the
NumPy restatement's time for two graphs of the kind on the same host (a Python loop over edges: a statement of the arithmetic, not a competitor).
There is no earlier device path to compare against, so no speed-up is claimed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alignnet-3d_amd")]

INPUTS = (("12 nodes, window 4", 256, 12, 4), ("100 nodes, window 4", 256, 100, 4), ("25 nodes, fully connected", 64, 25, 24))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_rate.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    import alignnet3d
    from tests import pose_graph_ref as G
    from tests.helpers import small_cfg
    eng = alignnet3d.Engine(small_cfg(N=64, nb=12))
    rec = {"form": "z-constrained", "repeats": args.repeats, "inputs": []}
    for name, count, n, w in INPUTS:
        graphs = [G.track(n, w, 9000 + k, wrong=3)[0] for k in range(count)]
        eng.pose_graph_optimize(graphs[:2], threshold=G.MU_THRESHOLD)          # (first touch: module load, workspace)
        eng.pose_graph_optimize(graphs, threshold=G.MU_THRESHOLD)
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = eng.pose_graph_optimize(graphs, threshold=G.MU_THRESHOLD)
            times.append((time.perf_counter() - t0) * 1e3)
        lds = eng.get_option("pose_graph_lds_graphs")
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        eng.pose_graph_optimize(graphs, threshold=G.MU_THRESHOLD)
        kernel_ms = eng.profile_kernels().get("pose_graph", (0.0, 0))[0]
        eng.profile_read(reset=True)
        eng.profile_enable(False)
        t0 = time.perf_counter()
        refs = [G.optimize(g, threshold=G.MU_THRESHOLD) for g in graphs[:2]]
        ref_ms = (time.perf_counter() - t0) * 1e3 / 2
        solves = [o["solves"] for o in out]
        item = {"input": name, "graphs": count, "nodes": n, "window": w, "edges_per_graph": len(graphs[0]["i"]), "placement": "LDS" if lds == count else
                ("workspace" if lds == 0 else "%d LDS / %d workspace" % (lds, count - lds)), "chunks": eng.get_option("pose_graph_chunks"),
                "call_ms_median": float(np.median(times)), "call_ms_min": min(times), "call_ms_max": max(times), "kernel_ms": kernel_ms,
                "solves_mean": float(np.mean(solves)), "solves_max": int(max(solves)), "converged": sum(o["status"] == "CONVERGED" for o in out),
                "graphs_per_second": count / (np.median(times) * 1e-3), "restatement_ms_per_graph": ref_ms,
                "restatement_solves": [r["solves"] for r in refs], "device_solves_same_graphs": solves[:2]}
        rec["inputs"].append(item)
        print("%-28s %3d graphs  call %.2f ms (%.2f .. %.2f)  kernel %.2f ms  %s  solves %.1f (max %d)  restatement %.0f ms per graph" %
              (name, count, item["call_ms_median"], item["call_ms_min"], item["call_ms_max"], kernel_ms, item["placement"], item["solves_mean"],
               item["solves_max"], ref_ms), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    return rec


if __name__ == "__main__":
    main()
