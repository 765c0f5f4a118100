"""Times the codon stage on the two standing batches of synthetic coding DNA (256 families x 32 sequences x ~600 nt, 64 x
128 x ~900 nt: kalign_amd.synth.family protein families threaded back to codons from a seed, a few in-frame stops; fast
mode) and prints one JSON line per batch.

    python tools/codon_time.py [--shape 256x32x600] [--runs 5] [--out profiles/codon_time.jsonl]

  (a) device ms of the pack, the translate and the backtranslation (ka_cod_fam_stats);
  (b) wall ms of kalign_amd.codon.align_codon_families from the list of strings;
  (c) wall ms of what a caller did before the stage: the translate of tests/cod_restate.py in Python for every sequence,
      kalign_amd.prepare.align_families on the proteins, and the restatement's backtranslate in Python for every row.
After one warm-up of each, (c) and (b) alternate, --runs times each; the line carries every wall time, best and worst.
The rows of (b) and (c) are compared byte for byte before anything is timed.  (a) comes from a handle of its own per run
that backtranslates the protein rows (b) returned: align_codon_families closes the one it uses."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ["256x32x600", "64x128x900"]
STOPS = ("TAA", "TAG", "TGA")


def thread(rng, protein, codons_of, p_stop=0.01):
    """a coding sequence of the protein: a random codon per amino acid, a few in-frame stops, one at the end"""
    out = []
    for aa in protein:
        if rng.random_sample() < p_stop:
            out.append(STOPS[rng.randint(0, 3)])
        c = codons_of[aa]
        out.append(c[rng.randint(0, len(c))])
    out.append(STOPS[rng.randint(0, 3)])
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxNUCLEOTIDES (may be repeated)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    import cod_restate as cr
    from kalign_amd import codon, prepare, synth
    from util import Golden

    g = Golden("tree_prot32x200")                                  # the reference's protein scoring
    subm, scal = g.subm, g.scal
    codons_of = {}
    for c in cr.CODONS:
        if cr.AA[c] != "*":
            codons_of.setdefault(cr.AA[c], []).append(c)
    ctx = kalign_amd.Context(0)
    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        rng = np.random.RandomState(a.seed)
        fams = [[thread(rng, p, codons_of) for p in synth.family(n_seq, length // 3, seed=a.seed + k)] for k in range(n_fam)]

        def by_hand():
            t0 = time.perf_counter()
            prot = [[cr.translate(s)["protein"] for s in f] for f in fams]
            t1 = time.perf_counter()
            prows = prepare.align_families(ctx, prot, (subm, scal), biotype=0, n_threads=a.threads)
            t2 = time.perf_counter()
            rows = [[cr.backtranslate(r, s).encode() for r, s in zip(pr, f)] for pr, f in zip(prows, fams)]
            t3 = time.perf_counter()
            return (t3 - t0) * 1e3, rows, ((t1 - t0) * 1e3, (t3 - t2) * 1e3)

        def stage():
            t0 = time.perf_counter()
            rows, prows = codon.align_codon_families(ctx, fams, subm, scal, n_threads=a.threads, want_protein=True)
            ms = (time.perf_counter() - t0) * 1e3
            cod = ctx.family_codons(fams)
            cod.back(prows)
            st = cod.stats()
            cod.close()
            return ms, rows, st

        _, want, _ = by_hand()                                     # warm-up of both, and the results must not differ
        _, got, _ = stage()
        equal = got == want
        hand, new = [], []
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            hand.append(by_hand())
            new.append(stage())
        out = dict(tool="codon_time", date=datetime.date.today().isoformat(), families=n_fam, sequences=n_seq, nucleotides=length, mode="fast",
                   threads=a.threads, rows_equal=bool(equal), raw_bytes=new[0][2]["bytes"],
                   pack_ms=[round(x[2]["pack_ms"], 4) for x in new], translate_ms=[round(x[2]["translate_ms"], 4) for x in new],
                   back_ms=[round(x[2]["back_ms"], 4) for x in new],
                   launches=new[0][2]["launches"], syncs=new[0][2]["syncs"], back_launches=new[0][2]["back_launches"],
                   back_syncs=new[0][2]["back_syncs"],
                   stage_wall_ms=[round(x[0], 2) for x in new], by_hand_wall_ms=[round(x[0], 2) for x in hand],
                   by_hand_translate_ms=[round(x[2][0], 2) for x in hand], by_hand_backtranslate_ms=[round(x[2][1], 2) for x in hand])
        for k in ("pack_ms", "translate_ms", "back_ms", "stage_wall_ms", "by_hand_wall_ms", "by_hand_translate_ms", "by_hand_backtranslate_ms"):
            out[k + "_best_worst"] = [min(out[k]), max(out[k])]
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
