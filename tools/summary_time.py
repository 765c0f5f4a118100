"""Times the summary stage over a batch of families through ONE FamilySummary (Context.family_summary = ka_sum_fam:
create, columns, summary, consensus, keep, compact) against the loop of one handle per family over the same rows, on the
same context in the same process, and against the numpy restatement (tests/sum_restate.py) on the host; prints one JSON
line per shape.

    python tools/summary_time.py [--shape 256x32x200] [--runs 5] [--out profiles/summary_time.jsonl]

Without --shape: 256 families x 32 sequences x ~200 residues, 64 x 128 x ~300 and one alignment of 4096 x ~1200.  Per
family: random protein sequences of 0.8 .. 1.2 x the length at sorted random columns of a 15 % wider alignment -- made
here from a seed, nothing else is read.  After one warm-up of each -- whose results must be equal -- loop and batch
alternate, --runs times each.  The line carries, per phase of the batch handle, the device ms from the stage's events
(best, median, worst), the bytes the phase must read and write (computed from the shapes and the kept widths) and from
them GB/s at the median and its share of 8 TB/s; the wall ms of the calls through Python of batch and loop (best, median,
worst) and the loop's device ms summed over its handles; the wall ms of the same outputs through the restatement
(--host-runs times: best, median, worst).

--tie-probe adds, per shape, the column table's device ms on two inputs of that shape that differ only in whether a
column's highest count is tied: mostly-gap columns whose last four rows read ABAA (no tie) or ABAB (a tie settled by a
walk over nearly all rows, the tie rule's worst case)."""
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

SHAPES = ["256x32x200", "64x128x300", "1x4096x1200"]
PHASES = ("table_ms", "consensus_ms", "keep_ms", "compact_ms")
PEAK = 8.0e12
GAP_THR = 0.5


def random_family(rng, n, length, gap_p=0.15):
    alpha = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    lens = rng.randint(int(length * 0.8), int(length * 1.2) + 1, size=n)
    W = int(lens.max() * (1.0 + gap_p)) + 1
    rows = np.full((n, W), ord("-"), np.uint8)
    for r, L in enumerate(lens):
        rows[r, np.sort(rng.choice(W, size=L, replace=False))] = alpha[rng.randint(0, len(alpha), size=L)]
    return [r.tobytes() for r in rows]


def tie_family(n, w, tied):
    rows = np.full((n, w), ord("-"), np.uint8)
    rows[-4:, :] = np.frombuffer(b"ABAB" if tied else b"ABAA", np.uint8)[:, None]
    return [r.tobytes() for r in rows]


def phase_bytes(fams, new_widths):
    """what each phase must read and write, from the shapes"""
    cells = sum(len(f) * len(f[0]) for f in fams)
    cols = sum(len(f[0]) for f in fams)
    kept_cells = sum(len(f) * w for f, w in zip(fams, new_widths))
    kept = sum(new_widths)
    keep = cols * 4 + cols * 4 + cols * 4 + kept * 4              # gap counts in, flags out; flags in, kept columns out
    return dict(table_ms=cells + cols * 21,                      # rows in; four ints, one byte and one int64 per column out
                consensus_ms=cols * 9 + cols + len(fams),        # gaps, top count and character in; the rows out
                keep_ms=keep,
                compact_ms=keep + kept * 4 + kept_cells + kept_cells + sum(len(f) for f in fams))


def spread(xs):
    return dict(best=round(min(xs), 4), median=round(statistics.median(xs), 4), worst=round(max(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3, help="runs of the host restatement")
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--tie-probe", action="store_true")
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    import sum_restate as sr

    ctx = kalign_amd.Context(0)

    def device(fams):
        """every output of one handle over fams; wall ms of the calls, the handle's device ms per phase"""
        t0 = time.perf_counter()
        s = ctx.family_summary(fams)
        out = (s.summary(), s.consensus(0.5), s.keep(GAP_THR), s.compact(GAP_THR))
        wall = (time.perf_counter() - t0) * 1e3
        st = s.stats()
        s.close()
        return wall, out, {k: st[k] for k in PHASES}

    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        rng = np.random.RandomState(a.seed)
        fams = [random_family(rng, n_seq, length) for _ in range(n_fam)]

        def loop():
            wall, outs, dev = 0.0, [], dict.fromkeys(PHASES, 0.0)
            for f in fams:
                w, o, d = device([f])
                wall += w
                outs.append(o)
                for k in PHASES:
                    dev[k] += d[k]
            return wall, tuple([o[i][0] for o in outs] for i in range(4)), dev

        def same(x, y):
            return x[0] == y[0] and x[1] == y[1] and x[3] == y[3] and all(np.array_equal(p, q) for p, q in zip(x[2], y[2]))

        host_runs = []
        for _ in range(max(1, a.host_runs)):
            t0 = time.perf_counter()
            host = ([sr.summary(f) for f in fams], [sr.consensus(f, 0.5) for f in fams], [sr.keep(f, GAP_THR) for f in fams],
                    [sr.compact(f, GAP_THR) for f in fams])
            host_runs.append((time.perf_counter() - t0) * 1e3)
        host_ms = statistics.median(host_runs)
        _, want, _ = loop()                                        # warm-up of both, and the results must not differ
        _, got, _ = device(fams)
        equal = same(got, want) and same(got, host)
        loops, batches = [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            loops.append(loop())
            batches.append(device(fams))
        nbytes = phase_bytes(fams, [len(f[0]) for f in got[3]])
        med = {k: statistics.median([b[2][k] for b in batches]) for k in PHASES}
        out = dict(tool="summary_time", date=time.strftime("%Y-%m-%d"), families=n_fam, sequences=n_seq, length=length, runs=len(batches),
                   columns=sum(len(f[0]) for f in fams), row_bytes=sum(len(f) * len(f[0]) for f in fams), results_equal=bool(equal),
                   batch_device_ms={k: spread([b[2][k] for b in batches]) for k in PHASES},
                   phase_bytes=nbytes,
                   batch_gb_s={k: round(nbytes[k] / (med[k] * 1e-3) / 1e9, 2) for k in PHASES},
                   share_of_8tb_s={k: round(nbytes[k] / (med[k] * 1e-3) / PEAK, 5) for k in PHASES},
                   batch_wall_ms=spread([b[0] for b in batches]), loop_wall_ms=spread([x[0] for x in loops]),
                   loop_device_ms_median={k: round(statistics.median([x[2][k] for x in loops]), 4) for k in PHASES},
                   host_restatement_wall_ms=spread(host_runs))
        out["speedup_wall_over_loop"] = round(out["loop_wall_ms"]["median"] / out["batch_wall_ms"]["median"], 3)
        out["speedup_wall_over_restatement"] = round(host_ms / out["batch_wall_ms"]["median"], 3)
        if a.tie_probe:
            w = len(fams[0][0])
            probe = {}
            for name, tied in (("no_tie", False), ("late_tie", True)):
                fam = tie_family(n_seq, w, tied)
                device([fam] * n_fam)
                probe[name] = spread([device([fam] * n_fam)[2]["table_ms"] for _ in range(max(1, a.runs))])
            out["tie_probe_table_ms"] = probe
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
