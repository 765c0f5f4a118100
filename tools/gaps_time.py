"""Times the gap structure and the ungapped rows of a batch of families through ONE FamilySummary (Context.family_summary
= ka_sum_fam: gaps(), ungapped()) against the loop of one handle per family over the same rows, on the same context in the
same process, and against the restatement (tests/sum_gap_restate.py) on the host; prints one JSON line per shape.

    python tools/gaps_time.py [--shape 256x32x200] [--runs 5] [--out profiles/gaps_time.jsonl]

Without --shape: 256 families x 32 sequences x ~200 residues, 64 x 128 x ~300 and one alignment of 4096 x ~1200, the
seeded families of tools/summary_time.py.  After one warm-up of each -- whose results must be equal -- loop and batch
alternate, --runs times each.  The line carries the device ms of the row pass with the gappy pass and of the ungap pass
from gap_stats() (best, median, worst), the bytes each must move (the rows in, 16 bytes a row and the column table's gap
counts; the rows in and the characters out) and that as a share of 8 TB/s at the median, the wall ms of handle + gaps() +
ungapped() through Python for batch and loop, and the wall ms of the restatement (--host-runs times; 0 skips it).

The yardsticks are the same handle's own passes over the same rows in the same runs: the column table (stats()
table_ms) for the row pass, compact at a gap threshold of 0.5 (compact_ms) for the ungap pass.  The line says whether the
best run of each new pass is no worse than the worst run of its yardstick."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from summary_time import GAP_THR, PEAK, SHAPES, random_family, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1, help="runs of the host restatement (0: none)")
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    import sum_gap_restate as gr

    ctx = kalign_amd.Context(0)

    def strip(g):
        return [{k: v for k, v in d.items() if k != "rows"} for d in g]

    def device(fams, yardsticks=False):
        """gaps and ungapped rows of one handle over fams; wall ms of handle + gaps() + ungapped(), the device ms"""
        t0 = time.perf_counter()
        s = ctx.family_summary(fams)
        out = (s.gaps(), s.ungapped())
        wall = (time.perf_counter() - t0) * 1e3
        st = s.gap_stats()
        assert (st["gaps_launches"], st["gaps_syncs"], st["ungap_launches"], st["ungap_syncs"]) == (2, 1, 1, 1)
        dev = dict(gaps_ms=st["gaps_ms"], ungap_ms=st["ungap_ms"])
        if yardsticks:
            s.compact(GAP_THR)
            six = s.stats()
            dev.update(table_ms=six["table_ms"], compact_ms=six["compact_ms"])
        s.close()
        return wall, out, dev

    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        rng = np.random.RandomState(a.seed)
        fams = [random_family(rng, n_seq, length) for _ in range(n_fam)]

        def loop():
            wall, g, u, dev = 0.0, [], [], dict(gaps_ms=0.0, ungap_ms=0.0)
            for f in fams:
                w, o, d = device([f])
                wall += w
                g.append(o[0][0])
                u.append(o[1][0])
                for k in dev:
                    dev[k] += d[k]
            return wall, (g, u), dev

        host_runs, host = [], None
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            host = (strip([gr.gaps(f) for f in fams]), [gr.ungapped(f)[0] for f in fams])
            host_runs.append((time.perf_counter() - t0) * 1e3)
        _, want, _ = loop()                                        # warm-up of both, and the results must not differ
        _, got, _ = device(fams, yardsticks=True)
        equal = got == want
        if host is not None:
            equal = equal and got == host
        loops, batches = [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            loops.append(loop())
            batches.append(device(fams, yardsticks=True))
        rows = sum(len(f) for f in fams)
        cols = sum(len(f[0]) for f in fams)
        cells = sum(len(f) * len(f[0]) for f in fams)
        chars = sum(d["characters"] for d in got[0])
        nbytes = dict(gaps_ms=cells + 16 * rows + 4 * cols, ungap_ms=cells + chars + 16 * rows)
        dev = {k: spread([b[2][k] for b in batches]) for k in ("gaps_ms", "ungap_ms", "table_ms", "compact_ms")}
        out = dict(tool="gaps_time", date=time.strftime("%Y-%m-%d"), families=n_fam, sequences=n_seq, length=length, runs=len(batches),
                   rows=rows, columns=cols, row_bytes=cells, characters=chars, results_equal=bool(equal), host_checked=host is not None,
                   device_ms=dev, pass_bytes=nbytes,
                   gb_s={k: round(nbytes[k] / (dev[k]["median"] * 1e-3) / 1e9, 2) for k in nbytes},
                   share_of_8tb_s={k: round(nbytes[k] / (dev[k]["median"] * 1e-3) / PEAK, 5) for k in nbytes},
                   gaps_best_le_table_worst=bool(dev["gaps_ms"]["best"] <= dev["table_ms"]["worst"]),
                   ungap_best_le_compact_worst=bool(dev["ungap_ms"]["best"] <= dev["compact_ms"]["worst"]),
                   batch_wall_ms=spread([b[0] for b in batches]), loop_wall_ms=spread([x[0] for x in loops]),
                   loop_device_ms={k: spread([x[2][k] for x in loops]) for k in ("gaps_ms", "ungap_ms")})
        out["speedup_wall_over_loop"] = round(out["loop_wall_ms"]["median"] / out["batch_wall_ms"]["median"], 3)
        if host_runs:
            out["host_restatement_wall_ms"] = spread(host_runs)
            out["speedup_wall_over_restatement"] = round(out["host_restatement_wall_ms"]["median"] / out["batch_wall_ms"]["median"], 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
