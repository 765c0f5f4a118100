"""Times the input stage on the two standing batches (256 families x 32 sequences x ~200 residues, 64 x 128 x ~300;
synthetic protein families, kalign_amd.synth.family from a seed; fast mode) and prints one JSON line per batch.

    python tools/input_time.py [--shape 256x32x200] [--runs 5] [--out profiles/input_time.jsonl]

  (a) device ms of the scan and of the encode (ka_in_fam_stats);
  (b) wall ms of kalign_amd.prepare.align_families from the list of strings;
  (c) wall ms of what a caller did before the stage: guide.encode_tree / guide.encode of every sequence, the sort by
      length and index in Python, Context.run_families, and putting the rows back in input order.
After one warm-up of each, (c) and (b) alternate, --runs times each; the line carries every wall time, best and worst.
The rows of (b) and (c) are compared byte for byte before anything is timed."""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ["256x32x200", "64x128x300"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    from kalign_amd import guide, prepare, synth
    from util import Golden

    g = Golden("tree_prot32x200")                                  # the reference's protein scoring
    subm, scal = g.subm, g.scal
    ctx = kalign_amd.Context(0)
    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        fams = [synth.family(n_seq, length, seed=a.seed + k) for k in range(n_fam)]

        def by_hand():
            t0 = time.perf_counter()
            enc, orders = [], []
            for seqs in fams:
                order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), i))
                s = [seqs[i] for i in order]
                enc.append((guide.encode_tree(s), guide.encode(s), s))
                orders.append(order)
            t1 = time.perf_counter()
            rows = ctx.run_families(enc, subm, scal, n_threads=a.threads)
            out = []
            for order, r in zip(orders, rows):
                back = [None] * len(order)
                for p, i in enumerate(order):
                    back[i] = r[p]
                out.append(back)
            return (time.perf_counter() - t0) * 1e3, out, (t1 - t0) * 1e3

        def stage():
            t0 = time.perf_counter()
            rows, inp = prepare.align_families(ctx, fams, (subm, scal), n_threads=a.threads, want_input=True)
            ms = (time.perf_counter() - t0) * 1e3
            st = inp.stats()
            inp.close()
            return ms, rows, st

        _, want, _ = by_hand()                                     # warm-up of both, and the results must not differ
        _, got, _ = stage()
        equal = got == want
        hand, new = [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            hand.append(by_hand())
            new.append(stage())
        out = dict(tool="input_time", date=datetime.date.today().isoformat(), families=n_fam, sequences=n_seq, length=length, mode="fast",
                   threads=a.threads, rows_equal=bool(equal), raw_bytes=new[0][2]["bytes"],
                   scan_ms=[round(x[2]["scan_ms"], 4) for x in new], encode_ms=[round(x[2]["encode_ms"], 4) for x in new],
                   launches=new[0][2]["launches"], syncs=new[0][2]["syncs"],
                   stage_wall_ms=[round(x[0], 2) for x in new], by_hand_wall_ms=[round(x[0], 2) for x in hand],
                   by_hand_encode_sort_ms=[round(x[2], 2) for x in hand], stage_run_wall_ms=[round(x[2]["run_wall_ms"], 2) for x in new])
        for k in ("scan_ms", "encode_ms", "stage_wall_ms", "by_hand_wall_ms", "by_hand_encode_sort_ms", "stage_run_wall_ms"):
            out[k + "_best_worst"] = [min(out[k]), max(out[k])]
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
