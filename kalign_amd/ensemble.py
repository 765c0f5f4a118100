"""The end of an ensemble: kalign_ensemble's stage after the members (lib/src/ensemble.c:341-497) on the device.

finish_ensemble takes the members' rows (dist.ensemble_members returns them) and does what the reference does with them:
scores every member, picks one, tries the consensus alignment, refines the winner, and computes confidences."""
from .api import KalignAmdError, residue_lens


def auto_min_support(n_runs):
    """kalign_ensemble's min_support when the caller gives none (ensemble.c:393-394)"""
    return max(2, (n_runs + 2) // 3)


def select(scores):
    """score_alignments' choice (ensemble.c:121-127): member 0 unless a later one beats the best so far and member 0 by > 5 %"""
    best = 0
    for k in range(1, len(scores)):
        if scores[k] > scores[best] and scores[k] > scores[0] * 1.05:
            best = k
    return best


def finish_ensemble(ctx, member_rows, letters, min_support=0, rerun_refined=None, save_poar_path=None):
    """member_rows[k]: the rows of member k (bytes / str, one per sequence, input order); letters: the sequences.
    min_support > 0: the consensus at that threshold, no selection (as kalign_ensemble with an explicit min_support).
    min_support == 0: the consensus at auto_min_support(n_runs) wins if it scores higher than the selected member; else,
    when rerun_refined is given, rerun_refined(best_k) must return member best_k's rows re-run with refine mode 2
    (KALIGN_REFINE_CONFIDENT, the member's gap penalties and tree noise -- whose multipliers come from the caller's RNG)
    and they replace the member if they score higher.
    save_poar_path: the members' POAR table goes to that file after the member scores, where kalign_ensemble writes it
    (ensemble.c:349-355; poar_table_write's bytes); consensus_from_poar reads it back.  Nothing else changes.
    Returns a dict: rows (bytes), residue_confidence (float32[n, width]), column_confidence (float32[width]), scores
    (per member), best_k, use_consensus, consensus_score (None when not computed), refined_score (None when not run),
    refined (whether the refined rows were kept)."""
    n_runs = len(member_rows)
    if n_runs < 1:
        raise KalignAmdError("an ensemble needs members")
    letters = [x.encode() if isinstance(x, str) else bytes(x) for x in letters]
    lens = residue_lens(letters)
    ens = ctx.ensemble(lens, n_runs)
    try:
        for k, rows in enumerate(member_rows):
            ens.add_member(k, rows)
        scores = [ens.score(rows)[1] for rows in member_rows]
        best_k = select(scores)
        if save_poar_path is not None:
            ens.write_table(save_poar_path)
        out = dict(scores=scores, best_k=best_k, use_consensus=False, consensus_score=None, refined_score=None, refined=False)
        chosen = [bytes(r.encode() if isinstance(r, str) else r) for r in member_rows[best_k]]
        if min_support > 0:
            chosen = ens.consensus(letters, int(min_support))
            out["use_consensus"] = True
        else:
            cons = ens.consensus(letters, auto_min_support(n_runs))
            out["consensus_score"] = ens.score(cons)[1]
            if out["consensus_score"] > scores[best_k]:
                chosen = cons
                out["use_consensus"] = True
        if not out["use_consensus"] and rerun_refined is not None:
            refined = [bytes(r.encode() if isinstance(r, str) else r) for r in rerun_refined(best_k)]
            out["refined_score"] = ens.score(refined)[1]
            if out["refined_score"] > scores[best_k]:
                chosen = refined
                out["refined"] = True
        out["rows"] = chosen
        out["residue_confidence"], out["column_confidence"] = ens.confidence(chosen)
        out["stats"] = ens.stats()
        return out
    finally:
        ens.close()


def finish_ensembles(ctx, member_rows, letters, min_support=0, rerun_refined=None, n_threads=4):
    """finish_ensemble for a batch of families with the same number of members, in a number of launches that does not grow
    with the batch (Context.family_ensemble).  member_rows[k][f]: the rows of member k of family f (what k calls of
    Context.run_families return); letters[f]: the sequences of family f.  min_support as finish_ensemble's, for every family.
    rerun_refined(list of (f, best_k)) is asked once, for the families whose selected member beat the consensus, and
    returns their refined rows in that order (rerun_refined_batch builds one over Context.run_families(refine=2)).
    n_threads: host threads of the consensus (1..16).
    Returns one dict per family with finish_ensemble's keys, each equal to finish_ensemble run on that family alone
    (stats: the batch's, the same dict in every family)."""
    n_runs = len(member_rows)
    if n_runs < 1:
        raise KalignAmdError("an ensemble needs members")
    letters = [[x.encode() if isinstance(x, str) else bytes(x) for x in f] for f in letters]
    F = len(letters)
    ens = ctx.family_ensemble([residue_lens(f) for f in letters], n_runs)
    try:
        for k, fams in enumerate(member_rows):
            ens.add_member(k, fams)
        scores = ens.score_members()[1]
        outs = []
        for f in range(F):
            sc = [float(scores[k, f]) for k in range(n_runs)]
            outs.append(dict(scores=sc, best_k=select(sc), use_consensus=False, consensus_score=None, refined_score=None, refined=False))
        chosen = [[bytes(r.encode() if isinstance(r, str) else r) for r in member_rows[o["best_k"]][f]] for f, o in enumerate(outs)]
        if min_support > 0:
            chosen = ens.consensus(letters, int(min_support), n_threads)
            for o in outs:
                o["use_consensus"] = True
        else:
            cons = ens.consensus(letters, auto_min_support(n_runs), n_threads)
            cscore = ens.score(cons)[1]
            for f, o in enumerate(outs):
                o["consensus_score"] = float(cscore[f])
                if o["consensus_score"] > o["scores"][o["best_k"]]:
                    chosen[f] = cons[f]
                    o["use_consensus"] = True
        ask = [(f, o["best_k"]) for f, o in enumerate(outs) if not o["use_consensus"]]
        if ask and rerun_refined is not None:
            refined = [[bytes(r.encode() if isinstance(r, str) else r) for r in rows] for rows in rerun_refined(ask)]
            if len(refined) != len(ask):
                raise KalignAmdError("rerun_refined returned %d alignments for %d families" % (len(refined), len(ask)))
            rows = [None] * F
            for (f, _), r in zip(ask, refined):
                rows[f] = r
            rscore = ens.score(rows)[1]
            for (f, k), r in zip(ask, refined):
                outs[f]["refined_score"] = float(rscore[f])
                if outs[f]["refined_score"] > outs[f]["scores"][k]:
                    chosen[f] = r
                    outs[f]["refined"] = True
        conf = ens.confidence(chosen)
        stats = ens.stats()
        for f, o in enumerate(outs):
            o["rows"] = chosen[f]
            o["residue_confidence"], o["column_confidence"] = conf[f]
            o["stats"] = stats
        return outs
    finally:
        ens.close()


def rerun_refined_batch(ctx, families, subm, member, ranks=None, **run_kw):
    """A rerun_refined for finish_ensembles: the selected members re-run with refine mode 2 (KALIGN_REFINE_CONFIDENT, as
    kalign_ensemble re-runs them, ensemble.c:403-451) through Context.run_families -- one batch call per distinct
    member, since a batch call holds one scal.
    families[f]: (tree_codes, codes, letters) as run_families takes them; member(k, fs) is the caller's and returns
    (scal_k, dm_scale) for member k and the families fs (a list of indices into families): the member's scoring and None
    or one block of n * min(32, n) guide-tree multipliers per family of fs (the random numbers stay the caller's);
    ranks[f], when given, maps family f's rows back to input order (row i belongs to input sequence ranks[f][i]), which
    is what finish_ensembles takes; run_kw goes to run_families (n_anchors, weight, realign, n_threads, gap).
    The callable returned takes [(f, best_k), ...] and returns those families' rows in that order."""
    def rerun(ask):
        ask = [(int(f), int(k)) for f, k in ask]
        by_member = {}
        for f, k in ask:
            if f in by_member.setdefault(k, []):
                raise KalignAmdError("rerun_refined_batch: family %d is asked for twice with member %d" % (f, k))
            by_member[k].append(f)
        rows = {}
        for k in sorted(by_member):
            fs = by_member[k]
            scal_k, dm_scale = member(k, list(fs))
            got = ctx.run_families([families[f] for f in fs], subm, scal_k, dm_scale=dm_scale, refine=2, **run_kw)
            for f, r in zip(fs, got):
                if ranks is not None:
                    back = [None] * len(r)
                    for i, x in enumerate(ranks[f]):
                        back[int(x)] = r[i]
                    r = back
                rows[(f, k)] = r
        return [rows[fk] for fk in ask]
    return rerun


def consensus_from_poar(ctx, letters, poar_path, min_support):
    """kalign_consensus_from_poar (ensemble.c:500-543): the consensus alignment at min_support and its confidences from a
    saved POAR table, no members at hand.  letters: the sequences, in the order of the run that wrote the table.
    Returns a dict: rows (bytes), residue_confidence, column_confidence, n_runs (the file's), stats."""
    if int(min_support) < 1:
        raise KalignAmdError("min_support must be >= 1")
    letters = [x.encode() if isinstance(x, str) else bytes(x) for x in letters]
    ens = ctx.ensemble_from_table(residue_lens(letters), path=poar_path)
    try:
        rows = ens.consensus(letters, int(min_support))
        res, col = ens.confidence(rows)
        return dict(rows=rows, residue_confidence=res, column_confidence=col, n_runs=ens.n_runs, stats=ens.stats())
    finally:
        ens.close()


def extend_poar(ctx, letters, poar_path, member_rows, save_poar_path=None, min_support=0):
    """A saved POAR table grown by new members, the old members not run again: the table of poar_path merged with the
    table of member_rows (Ensemble.merge), the new members numbered after the old ones as kalign_ensemble numbers member k.
    letters: the sequences, in the order of the run that wrote the table; save_poar_path: the merged table goes to that
    file.  The new members are scored against the merged table (the old members' rows are in no table, so no member is
    selected); the consensus is taken at min_support, or at auto_min_support(n_runs) of the merged table when it is 0.
    Returns a dict: rows (bytes), residue_confidence, column_confidence, n_runs (old and new), n_old, scores (of the new
    members), stats."""
    if len(member_rows) < 1:
        raise KalignAmdError("an ensemble needs members")
    if int(min_support) < 0:
        raise KalignAmdError("min_support must be >= 0")
    letters = [x.encode() if isinstance(x, str) else bytes(x) for x in letters]
    lens = residue_lens(letters)
    old = new = merged = None
    try:
        old = ctx.ensemble_from_table(lens, path=poar_path)
        new = ctx.ensemble(lens, len(member_rows))
        for k, rows in enumerate(member_rows):
            new.add_member(k, rows)
        merged = old.merge(new)
        if save_poar_path is not None:
            merged.write_table(save_poar_path)
        scores = [merged.score(rows)[1] for rows in member_rows]
        rows = merged.consensus(letters, int(min_support) if min_support > 0 else auto_min_support(merged.n_runs))
        res, col = merged.confidence(rows)
        return dict(rows=rows, residue_confidence=res, column_confidence=col, n_runs=merged.n_runs, n_old=old.n_runs,
                    scores=scores, stats=merged.stats())
    finally:
        for e in (merged, new, old):
            if e is not None:
                e.close()
