"""Times a batch of families through ONE call (Context.run_families = ka_run_encoded_batch) against a loop of
run_encoded over the same families, on the same context in the same process, and prints one JSON line per case.

    python tools/families_time.py [--shape 256x32x200] [--mode fast|default|realign] [--refine 2] [--runs 3] [--out profiles/families_time.jsonl]

Without --shape / --mode: both batch shapes (256 families x 32 sequences x ~200 residues, 64 x 128 x ~300; synthetic
protein families, kalign_amd.synth.family from a seed) in all three modes (--fast; the default mode, 5 anchors; the
default mode with one realignment).  --refine R: the refinement mode of both sides (run_encoded's / run_families' refine: 1, 2
KALIGN_REFINE_CONFIDENT, | 256 adaptive budget, 3 inline; default 0, none); with 2 the line also carries how many edges the
families' own medians marked (ka_batch_refine_stats).  The loop uses run_encoded only, so it is what a caller had before the batch call.
After one warm-up of each, loop and batch alternate, --runs times each; the line carries every wall time and the
medians, the batch's device ms per stage (ka_batch_stats: guide-tree distance batches, alignment runs, realignment
distances + UPGMA, rows), and for the loop the device ms of every family's LAST alignment run (ka_tree_kernel_ms: the
only stage time run_encoded leaves behind).  The rows of both are compared byte for byte before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ["256x32x200", "64x128x300"]
MODES = {"fast": dict(n_anchors=0, realign=0), "default": dict(n_anchors=5, realign=0), "realign": dict(n_anchors=5, realign=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--mode", action="append", choices=sorted(MODES))
    ap.add_argument("--refine", type=int, default=0, help="refinement mode of both sides (0 none, 1, 2, | 256, 3)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    from kalign_amd import guide, synth
    from util import Golden

    g = Golden("tree_prot32x200")                                  # the reference's protein scoring
    subm, scal = g.subm, g.scal
    ctx = kalign_amd.Context(0)
    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        fams = []
        for k in range(n_fam):
            seqs = synth.family(n_seq, length, seed=a.seed + k)
            fams.append((guide.encode_tree(seqs), guide.encode(seqs), seqs))
        for mode in a.mode or ["fast", "default", "realign"]:
            kw = dict(MODES[mode], refine=a.refine)

            def loop():
                t0 = time.perf_counter()
                rows, dp = [], 0.0
                for f in fams:
                    rows.append(ctx.run_encoded(f[0], f[1], f[2], subm, scal, weight=2.0, n_threads=a.threads, **kw))
                    dp += ctx.tree_kernel_ms()[0]
                return (time.perf_counter() - t0) * 1e3, rows, dp

            def batch():
                t0 = time.perf_counter()
                rows = ctx.run_families(fams, subm, scal, weight=2.0, n_threads=a.threads, **kw)
                return (time.perf_counter() - t0) * 1e3, rows, ctx.batch_stats()

            _, want, _ = loop()                                    # warm-up of both, and the results must not differ
            _, got, _ = batch()
            equal = got == want
            loops, batches = [], []
            for _ in range(max(1, a.runs)):                        # alternating: other work shares the host
                loops.append(loop())
                batches.append(batch())
            stats = [b[2] for b in batches]
            med = lambda xs: statistics.median(xs)                 # noqa: E731
            out = dict(tool="families_time", families=n_fam, sequences=n_seq, length=length, mode=mode, refine=a.refine, threads=a.threads,
                       rows_equal=bool(equal),
                       loop_wall_ms=[round(x[0], 2) for x in loops], batch_wall_ms=[round(x[0], 2) for x in batches],
                       loop_wall_ms_median=round(med([x[0] for x in loops]), 2),
                       batch_wall_ms_median=round(med([x[0] for x in batches]), 2),
                       loop_last_run_dp_ms_median=round(med([x[2] for x in loops]), 3),
                       batch_device_ms_median={k: round(med([s[k] for s in stats]), 3)
                                               for k in ("guide_dist_ms", "dp_ms", "realign_tree_ms", "rows_ms")},
                       batch_call_ms_median=round(med([s["wall_ms"] for s in stats]), 2), batch_jobs=stats[0]["jobs"])
            out["speedup_wall"] = round(out["loop_wall_ms_median"] / out["batch_wall_ms_median"], 3)
            if a.refine & 255 == 2:
                st = ctx.batch_refine_stats(n_fam)
                out["edges"], out["refined_edges"] = int(st["edges"].sum()), int(st["refined"].sum())
            line = json.dumps(out)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
