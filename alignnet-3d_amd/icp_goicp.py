#!/usr/bin/env python3
"""Go-ICP registration of the val pairs on the GPU: the `goicp` ICP baseline that the reference names (icp.py:146-147, called at :188-189
with `refine` and refine_radius=0.10) and leaves `assert False`: a branch-and-bound over yaw and a translation box on subsampled working
sets, independent of any start, with a lower bound on what any pose of the box can reach (tests/goicp_ref.py defines it).

    python icp_goicp.py --config configs/icp_<dataset>_goicp.json [--use_old_results]

The twin of icp_global.py: it writes into <logdir>/val/eval000000 what train.py's ICP mode writes (pred_translations.npy = T[:3, 3],
pred_angles.npy = the z component of T's rotation vector, zero pred_s1_pc1centers.npy, eval.json / eval_180.json with mean_time =
registration wall time / nval).  With `refine: "p2p"` in the config, point-to-point ICP on the FULL clouds (radius 0.10, 30 iterations)
follows from the search's pose inside the same call, as the reference's signature has it; the fitness logged is then the refinement's,
otherwise the share of the source working set within 0.10 m of a target.  The search is z-constrained: with_constraint must be true, as
it is in every shipped ICP config.  The search's parameters are Engine.GOICP_DEFAULTS."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import icp_global_common as common  # noqa: E402
from icp_global_common import cfg  # noqa: E402

ACCEPTS = "icp_goicp.py accepts evaluation.special.mode = \"icp\" with icp.variant = \"goicp\", icp.with_constraint = true and icp.refine absent or \"p2p\""


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", required=True, help="Config file (icp_*_goicp.json)")
    p.add_argument("--use_old_results", action="store_true", help="Re-evaluate the stored results instead of registering")
    return p.parse_args(argv)


def check_config():
    special = cfg.evaluation.special if cfg.evaluation.has("special") else None
    if special is None or special.mode != "icp":
        raise ValueError("%s (this config has %s)" % (ACCEPTS, "no evaluation.special" if special is None else "mode = %r" % (special.mode,)))
    icp = special.icp
    refine = icp.refine if icp.has("refine") else None
    if icp.variant != "goicp" or refine not in (None, "p2p"):
        raise ValueError("%s (this config has variant = %r, refine = %r)" % (ACCEPTS, icp.variant, refine))
    if not bool(icp.with_constraint):
        raise ValueError("%s (this config has with_constraint = false: the search covers yaw and translation only)" % ACCEPTS)
    return icp


def run(flags):
    icp = check_config()
    refine = icp.refine if icp.has("refine") else None
    statuses = {}

    def register(engine, rows, streams, constrained):
        res = engine.goicp_register_rows(rows, constrained=constrained, refine=refine)
        for s in res["status"]:
            name = engine.GOICP_STATUS[int(s)]
            statuses[name] = statuses.get(name, 0) + 1
        return res

    common.run(flags, icp, "Go-ICP registration", "pairs", register,
               lambda constrained, nval, total_time, fitness: "Go-ICP registration (goicp: branch-and-bound over yaw and translation%s) on %d pairs: %.3f s, "
               "mean fitness %.3f, stop statuses %s" % (", then point-to-point ICP" if refine else "", nval, total_time, fitness, dict(sorted(statuses.items()))))


def main(argv=None):
    common.main(parse_args(argv), check_config, run)


if __name__ == "__main__":
    main()
