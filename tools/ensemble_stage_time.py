"""Times the ensemble consensus stage (ka_ens) at one size and prints one JSON line.

    python tools/ensemble_stage_time.py --n 512 [--length 300] [--runs 8] [--ref]

Members: synthetic disagreeing rows (tests/golden/make_golden_ensemble.synthetic: one base alignment, every member moves
residues across the gap runs next to them), numseq x ~length.  Reported: device ms of the position maps, of every member's
score, of the consensus' count and write passes per support level, of the consensus' score and of the confidence; host ms of
the greedy union and of the column order; candidates per level; with --ref, the reference's stage (POAR table over the
members, member scores, consensus, its score, confidence; oracle/_ref/libkalign_ref.so) on the same rows, and whether the
consensus rows agree."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ref", action="store_true", help="also time the reference's stage (slow beyond 512 sequences)")
    a = ap.parse_args()

    import kalign_amd
    import make_golden_ensemble as mg
    from kalign_amd import ensemble

    seqs, members = mg.synthetic(a.n, a.length, a.runs, a.seed, moves=8)
    ctx = kalign_amd.Context(0)
    min_sup = ensemble.auto_min_support(a.runs)
    out = dict(tool="ensemble_stage_time", numseq=a.n, length=a.length, runs=a.runs, min_support=min_sup,
               residues=sum(len(s) for s in seqs))
    t0 = time.perf_counter()
    e = ctx.ensemble([len(s) for s in seqs], a.runs)
    for k, rows in enumerate(members):
        e.add_member(k, rows)
    out["upload_host_ms"] = (time.perf_counter() - t0) * 1e3
    e.score(members[0])                                     # builds the maps, warms up the kernels
    out["maps_ms"] = e.stats()["maps_ms"]
    score_ms = []
    for rows in members:
        e.score(rows)
        score_ms.append(e.stats()["score_ms"])
    out["member_score_ms"] = score_ms
    t0 = time.perf_counter()
    cons = e.consensus(seqs, min_sup)
    out["consensus_wall_ms"] = (time.perf_counter() - t0) * 1e3
    st = e.stats()
    for k in ("count_ms", "write_ms", "greedy_host_ms", "columns_host_ms", "wait_host_ms", "chunks", "bfs_truncations"):
        out["consensus_" + k] = st[k]
    out["level_candidates"] = st["level_candidates"]
    out["level_device_ms"] = {L: round(v, 3) for L, v in st["level_ms"].items()}
    out["consensus_width"] = len(cons[0])
    e.score(cons)
    out["consensus_score_ms"] = e.stats()["score_ms"]
    e.confidence(cons)
    out["confidence_ms"] = e.stats()["confidence_ms"]
    e.close()
    ctx.close()
    out["device_ms_total"] = out["maps_ms"] + sum(score_ms) + st["count_ms"] + st["write_ms"] + out["consensus_score_ms"] + out["confidence_ms"]
    if a.ref:
        if not mg.available():
            out["ref"] = "oracle/_ref not built"
        else:
            t0 = time.perf_counter()
            t = mg.Table(members)
            t1 = time.perf_counter()
            for rows in members:
                t.score(rows)
            t2 = time.perf_counter()
            rcons = t.consensus(seqs, min_sup)
            t3 = time.perf_counter()
            t.score(rcons)
            t.confidence(seqs, rcons)
            t4 = time.perf_counter()
            t.close()
            out["ref_table_ms"] = (t1 - t0) * 1e3
            out["ref_scores_ms"] = (t2 - t1) * 1e3
            out["ref_consensus_ms"] = (t3 - t2) * 1e3
            out["ref_score_confidence_ms"] = (t4 - t3) * 1e3
            out["ref_stage_ms"] = (t4 - t0) * 1e3
            out["consensus_equal_to_ref"] = [x.decode() for x in cons] == rcons
    print(json.dumps(out))


if __name__ == "__main__":
    main()
