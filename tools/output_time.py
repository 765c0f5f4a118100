"""Times the output stage's four formats (ka_out_fam) on the two batches the other stages use, against the Python restatement
of tests/out_restate.py -- a loop over rows and lines, which is what the reference's writers are -- on the same host:

    python tools/output_time.py [--out profiles/output_time.jsonl]

Per format and batch, best .. worst of 5 runs after a warm-up: device ms of the row pass and of the fill from the handle's
stats; wall ms from lists of rows to a list of bytes through the Python binding (handle and call, and each alone; a later call
on a live handle); wall ms of the restatement.  The texts of both ways are compared before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import out_restate as orr  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()
import kalign_amd  # noqa: E402
from kalign_amd import api  # noqa: E402

DATE = b"October 21, 2026 18:00"                 # (the library never reads the clock)
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY----", np.uint8)


def batch(n_fam, n, length, seed):
    rng = np.random.default_rng(seed)
    fams, names = [], []
    for f in range(n_fam):
        w = int(length + rng.integers(-length // 10, length // 10 + 1))
        fams.append([rng.choice(LETTERS, size=w).tobytes() for _ in range(n)])
        names.append([b"fam%d_seq%d" % (f, i) for i in range(n)])
    return fams, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()
    ctx = kalign_amd.Context(0)
    for n_fam, n, length in ((256, 32, 200), (64, 128, 300)):
        fams, names = batch(n_fam, n, length, n_fam)
        rng = np.random.default_rng(1)
        res = [rng.random((len(r), len(r[0]))).astype(np.float32) for r in fams]
        col = [rng.random(len(r[0])).astype(np.float32) for r in fams]
        titles = [b"fam%d.msf" % f for f in range(n_fam)]
        formats = {
            "fasta": (lambda h: h.fasta(60), lambda: [orr.fasta(r, m, 60) for r, m in zip(fams, names)]),
            "clustal": (lambda h: h.clustal(), lambda: [orr.clustal(r, m, api.CLUSTAL_HEADER) for r, m in zip(fams, names)]),
            "msf": (lambda h: h.msf(titles, 0, DATE), lambda: [orr.msf(r, m, t, 0, DATE) for r, m, t in zip(fams, names, titles)]),
            "stockholm": (lambda h: h.stockholm(res, col), lambda: [orr.stockholm(r, m, res[f], col[f]) for f, (r, m) in enumerate(zip(fams, names))]),
        }
        for fmt, (dev, host) in formats.items():
            want = host()
            h = ctx.family_output(fams, names)                    # warm-up: code objects, allocations
            assert dev(h) == want
            h.close()
            wall, handle_ms, call_ms, fill_ms, rows_ms, counts = [], [], [], [], [], None
            for _ in range(5):
                t0 = time.perf_counter()
                h = ctx.family_output(fams, names)
                t1 = time.perf_counter()
                got = dev(h)
                t2 = time.perf_counter()
                st = h.stats()
                h.close()
                assert got == want
                wall.append((t2 - t0) * 1e3); handle_ms.append((t1 - t0) * 1e3); call_ms.append((t2 - t1) * 1e3)
                fill_ms.append(st["fill_ms"]); rows_ms.append(st["rows_ms"]); counts = (st["launches"], st["syncs"])
            # a second call on a live handle: what a caller pays per format after the first
            h = ctx.family_output(fams, names)
            dev(h)
            again = []
            for _ in range(5):
                t0 = time.perf_counter()
                dev(h)
                again.append((time.perf_counter() - t0) * 1e3)
            h.close()
            base = []
            for _ in range(5):
                t0 = time.perf_counter()
                host()
                base.append((time.perf_counter() - t0) * 1e3)
            rec = dict(tool="output_time", date=time.strftime("%Y-%m-%d"), families=n_fam, sequences=n, length=length, format=fmt,
                       text_bytes=sum(len(t) for t in want), texts_equal=True, launches=counts[0], syncs=counts[1],
                       rows_ms=[round(x, 4) for x in rows_ms], fill_ms=[round(x, 4) for x in fill_ms],
                       stage_wall_ms=[round(x, 2) for x in wall], handle_ms=[round(x, 2) for x in handle_ms], call_ms=[round(x, 2) for x in call_ms],
                       later_call_ms=[round(x, 2) for x in again], restatement_wall_ms=[round(x, 2) for x in base])
            for k in ("rows_ms", "fill_ms", "stage_wall_ms", "handle_ms", "call_ms", "later_call_ms", "restatement_wall_ms"):
                rec[k + "_best_worst"] = [min(rec[k]), max(rec[k])]
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            print(fmt, n_fam, rec["text_bytes"], "fill", rec["fill_ms_best_worst"], "rows", rec["rows_ms_best_worst"], "wall", rec["stage_wall_ms_best_worst"],
                  "(handle", rec["handle_ms_best_worst"], "call", rec["call_ms_best_worst"], "later", rec["later_call_ms_best_worst"], ") restatement",
                  rec["restatement_wall_ms_best_worst"], flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
