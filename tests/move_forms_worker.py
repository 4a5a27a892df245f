"""TEST INFRASTRUCTURE: the child process of tests/test_gpu_move_forms.py for the move stage's process-wide switches
(SGE_MOVE_GROUP, SGE_MOVE_PIPELINE_LISTS: launch_move reads them once per process, so they come in through the environment of a
fresh process).

    python tests/move_forms_worker.py --sizes 17,65 --thresholds=-1,0 --steps K --seed-base S --out FILE.npz

Builds the scene of tests/move_forms.py for every size and threshold, steps it K times and writes bodies, controllers, locomotion,
actions and palettes of every run into one .npz (keys "n<size>_t<threshold>_<array>"), beside the scheduling state behind the
last step (counts, built_for_next) as evidence of which launches the process took."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", required=True)
    ap.add_argument("--thresholds", required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--seed-base", type=int, required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import numpy as np
    import __graft_entry__
    import move_forms as mf

    sge = __graft_entry__.build()
    eng = sge.CharacterEngine(0)
    out = {}
    for n in (int(x) for x in args.sizes.split(",")):
        for thr in (int(x) for x in args.thresholds.split(",")):
            eng.set_option(sge.abi.OPT_HEAVY_THRESHOLD, thr)
            mf.scene(sge, eng, n, args.seed_base + n)
            eng.move_stats()
            for _ in range(args.steps):
                mf.step(sge, eng)
            eng.synchronize()
            key = "n%d_t%d_" % (n, thr)
            for name, a in eng.download(what=("bodies", "controllers", "locomotion", "actions")).items():
                out[key + name] = a
            out[key + "palettes"] = eng.palettes()[0]
            sched = eng.move_schedule()
            out[key + "counts"] = sched["counts"]
            out[key + "built_for_next"] = np.int32(sched["built_for_next"])
            stats = eng.move_stats()
            out[key + "overflow"], out[key + "sweepTrips"] = np.int64(stats.overflow), np.int64(stats.sweepTrips)
    np.savez(args.out, **out)
    eng.close()


if __name__ == "__main__":
    main()
