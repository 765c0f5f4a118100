"""Times the pairwise identity matrices of a batch of families through ONE FamilySummary (Context.family_summary =
ka_sum_fam: identity()) against the loop of one handle per family over the same rows, on the same context in the same
process, and against the numpy restatement (tests/sum_identity_restate.py) on the host; prints one JSON line per shape.

    python tools/identity_time.py [--shape 256x32x200] [--runs 5] [--baseline] [--out profiles/identity_time.jsonl]

Without --shape: 256 families x 32 sequences x ~200 residues, 64 x 128 x ~300 and one alignment of 4096 x ~1200, the
seeded families of tools/summary_time.py.  After one warm-up of each -- whose results must be equal -- loop and batch
alternate, --runs times each.  The line carries the device ms of the identity pass from identity_stats() (best, median,
worst), the pair-columns per second that follow (sum over the families of N (N + 1) / 2 x W), the bytes the pass must
write (16 per entry: two int32 and a double) and read (the rows once) and that as a share of 8 TB/s, the wall ms of
handle + identity() through Python for batch and loop, and the wall ms of the restatement (--host-runs times; 0 skips it).

--baseline also runs the realignment distance pass over the same rows in this process (Context.aln_guide_tree per family:
ka_aln_dist_kernel, one pair per thread and a byte at a time, then UPGMA).  Its kernel's duration is not reported by the
library: read it from one kernel trace of this tool,
    rocprofv3 --kernel-trace --stats -- python tools/identity_time.py --shape 1x4096x1200 --runs 1 --host-runs 0 --baseline
where sum_identity stands beside ka_aln_dist_kernel."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from summary_time import PEAK, SHAPES, random_family, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1, help="runs of the host restatement (0: none)")
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--baseline", action="store_true", help="also run the realignment distance pass over the same rows")
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    import sum_identity_restate as ir

    ctx = kalign_amd.Context(0)

    def device(fams):
        """the identity matrices of one handle over fams; wall ms of handle + identity(), device ms of the pass"""
        t0 = time.perf_counter()
        s = ctx.family_summary(fams)
        out = s.identity()
        wall = (time.perf_counter() - t0) * 1e3
        st = s.identity_stats()
        s.close()
        assert st["launches"] == 1 and st["syncs"] == 1
        return wall, out, st["identity_ms"]

    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        rng = np.random.RandomState(a.seed)
        fams = [random_family(rng, n_seq, length) for _ in range(n_fam)]

        def loop():
            wall, outs, dev = 0.0, [], 0.0
            for f in fams:
                w, o, d = device([f])
                wall += w
                outs.append(o[0])
                dev += d
            return wall, outs, dev

        host_runs, host = [], None
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            host = [ir.identity(f)[0] for f in fams]
            host_runs.append((time.perf_counter() - t0) * 1e3)
        _, want, _ = loop()                                        # warm-up of both, and the results must not differ
        _, got, _ = device(fams)
        equal = all(np.array_equal(x, y) for x, y in zip(got, want))
        if host is not None:
            equal = equal and all(np.array_equal(x, y) for x, y in zip(got, host))
        loops, batches = [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            loops.append(loop())
            batches.append(device(fams))
        if a.baseline:
            t0 = time.perf_counter()
            for f in fams:
                ctx.aln_guide_tree(f)
            baseline_wall = (time.perf_counter() - t0) * 1e3
        entries = sum(len(f) ** 2 for f in fams)
        pair_cols = sum(len(f) * (len(f) + 1) // 2 * len(f[0]) for f in fams)
        row_bytes = sum(len(f) * (len(f[0]) + 1) for f in fams)
        med = statistics.median([b[2] for b in batches])
        out = dict(tool="identity_time", date=time.strftime("%Y-%m-%d"), families=n_fam, sequences=n_seq, length=length, runs=len(batches),
                   columns=sum(len(f[0]) for f in fams), entries=entries, pair_columns=pair_cols, results_equal=bool(equal),
                   host_checked=host is not None,
                   identity_device_ms=spread([b[2] for b in batches]),
                   pair_columns_per_s=round(pair_cols / (med * 1e-3), 1),
                   bytes_written=16 * entries, bytes_read=row_bytes,
                   gb_s=round((16 * entries + row_bytes) / (med * 1e-3) / 1e9, 2),
                   share_of_8tb_s=round((16 * entries + row_bytes) / (med * 1e-3) / PEAK, 5),
                   batch_wall_ms=spread([b[0] for b in batches]), loop_wall_ms=spread([x[0] for x in loops]),
                   loop_device_ms=spread([x[2] for x in loops]))
        out["speedup_wall_over_loop"] = round(out["loop_wall_ms"]["median"] / out["batch_wall_ms"]["median"], 3)
        if host_runs:
            out["host_restatement_wall_ms"] = spread(host_runs)
            out["speedup_wall_over_restatement"] = round(statistics.median(host_runs) / out["batch_wall_ms"]["median"], 3)
        if a.baseline:
            out["baseline_aln_guide_tree_wall_ms"] = round(baseline_wall, 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
