#!/usr/bin/env python3
"""What per-character mesh variants cost and what distance LOD saves, on the flagship workload (10,000 characters of the 14,080-vertex
synthetic mesh over the synthetic terrain, full stage set, default overlap schedule).

Three contexts in ONE process, their repetitions interleaved a / b / c / a / b / c ... so that drift of the machine hits all alike:

  a  the uniform path, no variant uploaded (the yardstick)
  b  variants uploaded (full, half, quarter vertex count), every character in variant 0: (b) - (a) = plan kernel + indirection
  c  sge_lod_select in front of every tick, thresholds at the 10 % and 40 % quantiles of the spawn distances to the eye:
     a 10 / 30 / 60 % split over full / half / quarter (the plan of the last tick says what the split was)

Per repetition: `--steps` ticks timed by the host clock around a device synchronise (ms per step), then `--profiled` ticks with
SGE_OPT_PROFILE on (HIP events around every skin launch: ms per skin launch; for b and c that bracket holds the plan kernel too).
Fraction of 8 TB/s = algorithmic bytes / launch time / 8e12: 40 B per written vertex + the palettes + every variant's source
vertices (64 B each) once per group of four characters.

--refit puts the acceleration-structure refit into the step (SGE_STAGE_BLAS_REFIT behind the skin launch, two-launch form in all
three configurations; (a) is blas_refit_kernel, (b) and (c) one blas_refit_ragged_kernel per variant) and adds ms per refit from
sge_blas_profile_read over the same repetitions. Bytes of a refit: 12 (packed) B per vertex read + 24 B per box row written.
With --refit the variants are complete meshes of their own (the synthetic mesh at 11 x 10 and 11 x 5 vertices per bone: 7,040 and
3,520 vertices, each with its index buffer), not vertex subsets: a decimated subset keeps too few triangles to be a mesh.

Needs an MI355X; there is no fallback. Run it under a time limit of its own:
    timeout -k 10 600 python tools/lod_bench.py --out profiles/lod_bench.txt"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12
SOURCE_BYTES = 64  # per source vertex: position 12, normal 12, tangent 16, bone indices 8, weights 16


def make_context(sge, ybot, chars, variants, refit=False, overlap=1):
    A = sge.abi
    eng = sge.CharacterEngine(0)
    eng.set_option(A.OPT_OVERLAP_SKIN, overlap)
    eng.set_option(A.OPT_FUSE_BLAS_REFIT, 0)
    built, mesh = sge.crowd.upload_character_assets(eng, ybot)
    terrain = sge.crowd.upload_terrain(eng)
    state = sge.crowd.spawn_crowd(eng, ybot, chars, terrain, seed=1234, mode="ccd")
    counts = [mesh["positions"].shape[0]]
    eng.refit_rows = []
    if refit:
        eng.refit_rows.append(eng.blas_build(mesh["indices"]).entryCount + 1)
    if variants:
        full = dict(mesh, tangents=eng.mesh["tangents"])
        for v, keep in ((1, 0.5), (2, 0.25)):
            m = sge.crowd.synthetic_lod_mesh(eng, built, ybot, 11, 10 if v == 1 else 5) if refit else sge.assets.decimate_skinned_mesh(full, keep)
            eng.upload_mesh_variant(v, m)
            counts.append(m["positions"].shape[0])
            if refit:
                eng.refit_rows.append(eng.blas_variant_build(v, m["indices"]).entryCount + 1)
    return eng, state, counts


def algorithmic_bytes(per_variant, counts, bones, cpw=4):
    chars = sum(per_variant)
    written = sum(n * v for n, v in zip(per_variant, counts)) * 40
    source = sum(-(-n // cpw) * v for n, v in zip(per_variant, counts)) * SOURCE_BYTES
    return written + chars * bones * 64 + source


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chars", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--profiled", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--refit", action="store_true", help="SGE_STAGE_BLAS_REFIT in every step; reports ms per refit as well")
    ap.add_argument("--overlap", type=int, default=1, help="SGE_OPT_OVERLAP_SKIN; 0: serial order, a launch's events bracket the kernel by itself")
    ap.add_argument("--configs", default="abc", help="which of a, b, c to build and time (a kernel trace of one configuration: --configs c)")
    args = ap.parse_args()
    import __graft_entry__
    sge = __graft_entry__.build()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lod_bench: no GPU visible; nothing is measured on a CPU")
    A = sge.abi
    ybot = sge.assets.YBotAssets()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = {}
    for name, variants in (("a", False), ("b", True), ("c", True)):
        if name not in args.configs:
            continue
        ctx[name] = make_context(sge, ybot, args.chars, variants, args.refit, args.overlap)
    first = next(iter(ctx.values()))
    pos = first[1]["bodies"]["position"]
    eye = np.array([pos[:, 0].mean(), pos[:, 1].mean() + 10.0, pos[:, 2].min() - 20.0])
    dist = np.sqrt(((pos - eye) ** 2).sum(1))
    thresholds = np.quantile(dist, [0.10, 0.40]).astype(np.float32)
    say("# lod_bench: %d characters, mesh vertex counts %s, %d bones, eye %s, thresholds %s" %
        (args.chars, max((c[2] for c in ctx.values()), key=len), ybot.bone_count, np.round(eye, 2).tolist(), thresholds.tolist()))
    say("# SGE_OPT_OVERLAP_SKIN %d%s" % (args.overlap, ", refit stage in the step" if args.refit else ""))
    say("# %d repetitions, interleaved a b c; per repetition %d timed ticks (host clock), then %d ticks under SGE_OPT_PROFILE" %
        (args.reps, args.steps, args.profiled))

    def ticks(name, n):
        eng = ctx[name][0]
        for _ in range(n):
            if name == "c":
                eng.lod_select(eye, thresholds)
            eng.tick(stages=stages)

    stages = A.STAGE_ALL | (A.STAGE_BLAS_REFIT if args.refit else 0)
    for name in ctx:
        ticks(name, args.warmup)
        ctx[name][0].synchronize()
    step_ms = {k: [] for k in ctx}
    skin_ms = {k: [] for k in ctx}
    refit_ms = {k: [] for k in ctx}
    for rep in range(args.reps):
        for name in ctx:
            eng = ctx[name][0]
            eng.synchronize()
            t0 = time.perf_counter()
            ticks(name, args.steps)
            eng.synchronize()
            step_ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
            eng.set_option(A.OPT_PROFILE, 1)
            eng.profile_read(reset=True)
            if args.refit:
                eng.blas_profile(reset=True)
            ticks(name, args.profiled)
            eng.synchronize()
            st = eng.profile_read(reset=True)
            eng.set_option(A.OPT_PROFILE, 0)
            skin_ms[name].append(st.skin_ms / max(st.skin_launches, 1))
            if args.refit:
                ms, n = eng.blas_profile(reset=True)
                refit_ms[name].append(ms / max(n, 1))
            say("rep %d config %s: %.4f ms per step, %.4f ms per skin launch%s" % (rep, name, step_ms[name][-1], skin_ms[name][-1],
                                                                                  ", %.4f ms per refit" % refit_ms[name][-1] if args.refit else ""))

    split = {"a": [args.chars]}
    for name in ("b", "c"):
        if name in ctx:
            plan = ctx[name][0].skin_plan()
            assert plan.dropped == 0
            split[name] = list(plan.perVariant)[:3]
    say("")
    say("config  ms/step median (min..max)     ms/skin launch median (min..max)   characters per variant   algorithmic GB   fraction of 8 TB/s")
    for name in ctx:
        counts = ctx[name][2]
        nbytes = algorithmic_bytes(split[name], counts, ybot.bone_count)
        s, k = np.array(step_ms[name]), np.array(skin_ms[name])
        say("%-6s  %.4f (%.4f..%.4f)         %.4f (%.4f..%.4f)               %-22s   %.3f            %.3f" %
            (name, np.median(s), s.min(), s.max(), np.median(k), k.min(), k.max(), split[name], nbytes / 1e9, nbytes / (np.median(k) * 1e-3) / PEAK))
    if args.refit:
        say("")
        say("config  ms/refit median (min..max)     refit bytes read + written (MB)   fraction of 8 TB/s")
        for name in ctx:
            counts, rows = ctx[name][2], ctx[name][0].refit_rows
            nbytes = sum(n * (v * 12 + r * 24) for n, v, r in zip(split[name], counts, rows))
            k = np.array(refit_ms[name])
            say("%-6s  %.4f (%.4f..%.4f)          %.2f                             %.3f" %
                (name, np.median(k), k.min(), k.max(), nbytes / 1e6, nbytes / (np.median(k) * 1e-3) / PEAK))
        if "a" in ctx and "b" in ctx:
            ra, rb = np.array(refit_ms["a"]), np.array(refit_ms["b"])
            say("(b) - (a), medians: %.4f ms per refit; spread (max - min) of (a): %.4f ms: %s" %
                (np.median(rb) - np.median(ra), ra.max() - ra.min(), "inside" if np.median(rb) - np.median(ra) <= ra.max() - ra.min() else "OUTSIDE"))
    if "a" not in ctx or "b" not in ctx:
        return finish(ctx, args, lines)
    a, b = np.array(step_ms["a"]), np.array(step_ms["b"])
    ka, kb = np.array(skin_ms["a"]), np.array(skin_ms["b"])
    say("")
    say("(b) - (a), medians: %.4f ms per step, %.4f ms per skin launch; spread (max - min) of (a): %.4f ms per step, %.4f ms per skin launch" %
        (np.median(b) - np.median(a), np.median(kb) - np.median(ka), a.max() - a.min(), ka.max() - ka.min()))
    say("acceptance bar, (b) not slower than (a) by more than (a)'s own spread: %s on the step, %s on the skin launch" %
        ("met" if np.median(b) - np.median(a) <= a.max() - a.min() else "MISSED", "met" if np.median(kb) - np.median(ka) <= ka.max() - ka.min() else "MISSED"))
    finish(ctx, args, lines)


def finish(ctx, args, lines):
    for e, _, _ in ctx.values():
        e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
