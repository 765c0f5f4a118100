"""Times FamilyComparer.detail (ka_cmp_fam_detail: per-residue and per-column agreement of a batch of families with their
references) against the score call on the same handle and against the numpy restatement of the column correctness on the
host (tests/detail_restate.py: column_flags, the semantics of the reference's _column_correctness), and prints one JSON
line per shape.

    python tools/compare_detail_time.py [--shape 256x32x200] [--runs 5] [--out profiles/compare_detail_time.jsonl]

Without --shape: both batch shapes of tools/families_compare_time.py (256 families x 32 sequences x ~200 residues, 64 x
128 x ~300), made by its noisy_family from a seed.  After one warm-up of each -- the device's flags must equal the host's --
detail and score alternate, --runs times each; the line carries every wall time through the Python binding, the device ms
both report per stage, the launches and synchronisations of a detail call, and the host restatement's wall time (one
run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from families_compare_time import SHAPES, noisy_family  # noqa: E402


def span(xs, digits=3):
    return [round(min(xs), digits), round(max(xs), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import detail_restate as DR
    import kalign_amd

    ctx = kalign_amd.Context(0)
    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        rng = np.random.RandomState(a.seed)
        refs, tests = zip(*[noisy_family(rng, n_seq, length) for _ in range(n_fam)])
        t0 = time.perf_counter()
        want = [DR.column_flags(r, t) for r, t in zip(refs, tests)]
        host_ms = (time.perf_counter() - t0) * 1e3
        cmp = ctx.family_comparer(refs)
        got = cmp.detail(tests)                                    # warm-up of both
        cmp.score(tests)
        equal = all(np.array_equal(g["test_columns"]["correct"], w) for g, w in zip(got, want))
        detail_wall, score_wall, detail_dev, score_dev = [], [], [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            t0 = time.perf_counter()
            cmp.detail(tests)
            detail_wall.append((time.perf_counter() - t0) * 1e3)
            detail_dev.append(cmp.detail_stats())
            t0 = time.perf_counter()
            cmp.score(tests)
            score_wall.append((time.perf_counter() - t0) * 1e3)
            score_dev.append(cmp.stats())
        cmp.close()
        flags = np.concatenate(want)
        out = dict(tool="compare_detail_time", families=n_fam, sequences=n_seq, length=length, runs=len(detail_wall),
                   flags_equal_to_host=bool(equal), test_columns=int(len(flags)), correct_columns=int(flags.sum()),
                   residues=int(sum(len(g["res"]) for g in got)),
                   detail_wall_ms=span(detail_wall, 2), score_wall_ms=span(score_wall, 2), host_column_flags_wall_ms=round(host_ms, 1),
                   detail_device_ms={k: span([d[k] for d in detail_dev]) for k in ("maps_ms", "walk_ms", "columns_ms")},
                   score_device_ms={k: span([d[k] for d in score_dev]) for k in ("maps_ms", "walk_ms", "tc_ms")},
                   detail_launches=detail_dev[-1]["launches"], detail_syncs=detail_dev[-1]["syncs"])
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
