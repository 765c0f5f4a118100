"""Times the ensemble consensus stage of a batch of families through ONE FamilyEnsemble (ensemble.finish_ensembles =
ka_ens_fam: members, member scores, consensus, its score, confidences) against the loop of ensemble.finish_ensemble over
the same families, on the same context in the same process, and prints one JSON line per shape.

    python tools/families_ensemble_time.py [--shape 256x32x200] [--members 8] [--runs 3] [--out profiles/families_ensemble_time.jsonl]

Without --shape: both batch shapes of tools/families_time.py (256 families x 32 sequences x ~200 residues, 64 x 128 x
~300; synthetic protein families, kalign_amd.synth.family from a seed).  The members come from --members calls of
Context.run_families in the fast mode, member k with the gap penalties scaled by GAP_SCALES[k % 8] (the spread an
ensemble run uses; member 0 runs the defaults): the rows of a call are a member as they stand.  The loop makes one
Ensemble per family, adds its members, scores them, builds the consensus at the automatic threshold, scores it and
computes the confidences: what a caller had before the batch form.  After one warm-up of each -- whose results must be
equal, or the tool fails -- the loop and the batch (with 1, 4 and 16 host threads) alternate, --runs times each.  The
line carries every wall time, the medians, the device and host parts both report (the loop's summed over its families)
and the batch's launch and synchronisation counts."""
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

SHAPES = ["256x32x200", "64x128x300"]
THREADS = (1, 4, 16)
GAP_SCALES = [(1.0, 1.0, 1.0), (0.5, 1.5, 0.8), (1.5, 0.5, 1.2), (0.7, 0.7, 0.5), (1.4, 1.4, 1.5), (0.8, 1.2, 1.0), (1.3, 0.8, 0.7), (0.6, 1.0, 1.3)]
# (device ms, host ms) of the two handles' stats under one name each
LOOP_PARTS = dict(maps_ms="maps_ms", count_ms="count_ms", write_ms="write_ms", confidence_ms="confidence_ms",
                  greedy_host_ms=("greedy_host_ms", "columns_host_ms"), wait_host_ms="wait_host_ms", chunks="chunks")
BATCH_PARTS = dict(maps_ms="maps_ms", count_ms="count_ms", write_ms="write_ms", confidence_ms="confidence_ms",
                   greedy_host_ms="greedy_threads_host_ms", greedy_wall_host_ms="greedy_wall_host_ms", wait_host_ms="wait_host_ms",
                   chunks="chunks", candidates="candidates")


def same(a, b):
    """two lists of finish_ensemble dicts hold the same results (stats apart)"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        for k in ("scores", "best_k", "use_consensus", "consensus_score", "refined_score", "refined", "rows"):
            if x[k] != y[k]:
                return False
        for k in ("residue_confidence", "column_confidence"):
            if x[k].shape != y[k].shape or x[k].tobytes() != y[k].tobytes():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="FAMILIESxSEQUENCESxLENGTH (may be repeated)")
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()

    import kalign_amd
    from kalign_amd import ensemble, guide, synth
    from util import Golden

    g = Golden("tree_prot32x200")                                  # the reference's protein scoring
    ctx = kalign_amd.Context(0)
    med = statistics.median
    for shape in a.shape or SHAPES:
        n_fam, n_seq, length = (int(x) for x in shape.split("x"))
        letters, fams = [], []
        for k in range(n_fam):
            seqs = synth.family(n_seq, length, seed=a.seed + k)
            letters.append(seqs)
            fams.append((guide.encode_tree(seqs), guide.encode(seqs), seqs))
        members = []
        t0 = time.perf_counter()
        for k in range(a.members):
            scal = np.array(g.scal, np.float32).copy()
            scal[:3] *= np.array(GAP_SCALES[k % len(GAP_SCALES)], np.float32)
            members.append(ctx.run_families(fams, g.subm, scal, n_anchors=0, weight=2.0, realign=0))
        members_ms = (time.perf_counter() - t0) * 1e3

        def loop():
            t0 = time.perf_counter()
            out, parts = [], dict.fromkeys(LOOP_PARTS, 0.0)
            for f in range(n_fam):
                r = ensemble.finish_ensemble(ctx, [m[f] for m in members], letters[f])
                out.append(r)
                for k, src in LOOP_PARTS.items():
                    parts[k] += sum(r["stats"][s] for s in ((src,) if isinstance(src, str) else src))
            return (time.perf_counter() - t0) * 1e3, out, parts

        def batch(n_threads):
            t0 = time.perf_counter()
            out = ensemble.finish_ensembles(ctx, members, letters, n_threads=n_threads)
            wall = (time.perf_counter() - t0) * 1e3
            st = out[0]["stats"]
            return wall, out, {k: st[src] for k, src in BATCH_PARTS.items()}, {k: v for k, v in st.items() if k.endswith("_launches") or k.endswith("_syncs")}

        _, want, _ = loop()                                        # warm-up of both, and the results must not differ
        for t in THREADS:
            if not same(batch(t)[1], want):
                raise SystemExit("finish_ensembles (n_threads=%d) and the loop of finish_ensemble differ at %s" % (t, shape))
        loops, batches = [], {t: [] for t in THREADS}
        for _ in range(max(1, a.runs)):                            # alternating: other work shares the host
            loops.append(loop())
            for t in THREADS:
                batches[t].append(batch(t))
        out = dict(tool="families_ensemble_time", families=n_fam, sequences=n_seq, length=length, members=a.members, results_equal=True,
                   members_run_families_wall_ms=round(members_ms, 1),
                   loop_wall_ms=[round(x[0], 1) for x in loops], loop_wall_ms_median=round(med([x[0] for x in loops]), 1),
                   loop_parts_ms_median={k: round(med([x[2][k] for x in loops]), 2) for k in LOOP_PARTS})
        for t in THREADS:
            b = batches[t]
            out["batch_t%d" % t] = dict(wall_ms=[round(x[0], 1) for x in b], wall_ms_median=round(med([x[0] for x in b]), 1),
                                        parts_ms_median={k: round(med([x[2][k] for x in b]), 2) for k in BATCH_PARTS},
                                        speedup_wall=round(out["loop_wall_ms_median"] / med([x[0] for x in b]), 2))
        out["batch_launches_syncs"] = batches[THREADS[0]][-1][3]
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
