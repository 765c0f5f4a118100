"""Times the scoring of a batch of families, each against its own reference alignment, through ONE FamilyComparer
(Context.family_comparer = ka_cmp_fam: create, set masks, score) against the loop of ctx.comparer(ref).score(test) over
the same families, on the same context in the same process, and prints one JSON line per shape.

    python tools/families_compare_time.py [--shape 256x32x200] [--runs 3] [--frac 0.2] [--out profiles/families_compare_time.jsonl]

Without --shape: both batch shapes of tools/families_time.py (256 families x 32 sequences x ~200 residues, 64 x 128 x
~300).  Per family: random protein sequences of 0.8 .. 1.2 x the length, a random alignment of them (the reference) and
a noisy copy (the test: 30 % of every row's residues moved inside their gap runs) -- made here from a seed, nothing else
is read.  Every second family is scored with a random partial column mask, the others with --frac.  The loop makes,
scores and closes one Comparer per family: what a caller had before the batch form.  After one warm-up of each -- whose
results must be equal -- loop and batch alternate, --runs times each; the line carries every wall time, the medians, the
device ms both report (the references' maps, the test maps, the walk, TC; the loop's summed over its families) and the
wall time of a further score() on the batch's handle (the references stay: what a second parameter set costs)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["256x32x200", "64x128x300"]
STAGES = ("ref_maps_ms", "maps_ms", "walk_ms", "tc_ms")


def noisy_family(rng, n, length, gap_p=0.15, noise=0.3):
    """(reference rows, test rows) as bytes: n random sequences, each at sorted random columns of the reference; in the
    test a share `noise` of every row's residues moved to a random free place between their neighbours"""
    alpha = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    lens = rng.randint(int(length * 0.8), int(length * 1.2) + 1, size=n)
    W = int(lens.max() * (1.0 + gap_p)) + 1
    ref, test = [], []
    for L in lens:
        cols = np.sort(rng.choice(W, size=L, replace=False))
        row = np.full(W, ord("-"), np.uint8)
        letters = alpha[rng.randint(0, len(alpha), size=L)]
        row[cols] = letters
        ref.append(row.tobytes())
        cols = cols.copy()
        for k in rng.randint(0, L, size=int(noise * L)):
            lo = cols[k - 1] + 1 if k > 0 else 0
            hi = cols[k + 1] - 1 if k + 1 < L else W - 1
            cols[k] = rng.randint(lo, hi + 1)
        row = np.full(W, ord("-"), np.uint8)
        row[cols] = letters
        test.append(row.tobytes())
    return ref, test


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frac", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd

    ctx = kalign_amd.Context(0)
    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        rng = np.random.RandomState(a.seed)
        refs, tests = zip(*[noisy_family(rng, n_seq, length) for _ in range(n_fam)])
        masks = [(rng.rand(len(r[0])) < 0.6).astype(np.int32) if f % 2 else None for f, r in enumerate(refs)]

        def loop():
            t0 = time.perf_counter()
            out, dev = [], dict.fromkeys(STAGES, 0.0)
            for r, t, m in zip(refs, tests, masks):
                cmp = ctx.comparer(r)
                out.append(cmp.score(t, max_gap_frac=a.frac, column_mask=m))
                for k, v in cmp.stats().items():
                    dev[k] += v
                cmp.close()
            return (time.perf_counter() - t0) * 1e3, out, dev

        def batch():
            t0 = time.perf_counter()
            cmp = ctx.family_comparer(refs)
            out = cmp.score(tests, max_gap_frac=a.frac, column_masks=masks)
            wall = (time.perf_counter() - t0) * 1e3
            dev = cmp.stats()
            t0 = time.perf_counter()
            cmp.score(tests, max_gap_frac=a.frac, column_masks=masks)
            again = (time.perf_counter() - t0) * 1e3
            cmp.close()
            return wall, out, dev, again

        _, want, _ = loop()                                        # warm-up of both, and the results must not differ
        _, got, _, _ = batch()
        equal = got == want
        loops, batches = [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            loops.append(loop())
            batches.append(batch())
        med = statistics.median
        out = dict(tool="families_compare_time", families=n_fam, sequences=n_seq, length=length, frac=a.frac,
                   results_equal=bool(equal),
                   loop_wall_ms=[round(x[0], 2) for x in loops], batch_wall_ms=[round(x[0], 2) for x in batches],
                   loop_wall_ms_median=round(med([x[0] for x in loops]), 2),
                   batch_wall_ms_median=round(med([x[0] for x in batches]), 2),
                   batch_score_again_wall_ms_median=round(med([x[3] for x in batches]), 2),
                   loop_device_ms_median={k: round(med([x[2][k] for x in loops]), 3) for k in STAGES},
                   batch_device_ms_median={k: round(med([x[2][k] for x in batches]), 3) for k in STAGES})
        out["speedup_wall"] = round(out["loop_wall_ms_median"] / out["batch_wall_ms_median"], 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
