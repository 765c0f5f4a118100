"""A CPU stand-in for kalign_amd.Context's partial-run interface, built from the oracle's per-task
primitives (tests only).  It lets the world_size-2 gloo test exercise kalign_amd.dist.sharded_tree --
the subtree plan, the profile hand-over between ranks and the final gather -- without a GPU."""
import ctypes as C

import numpy as np

from oracle import oracledrv


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def task_penalties(scal, gap_scale, subm_off):
    """(gpo, gpe, tgpe, soff) of one task as do_align scales them (aln_run.c:226-237), in fp32"""
    gs, soff = np.float32(gap_scale), np.float32(subm_off)
    gpo, gpe, tgpe = (np.float32(x) for x in scal[:3])
    if gs < 1.0 or soff > 0.0:
        return np.float32(gpo * gs), np.float32(gpe * gs), np.float32(tgpe * gs), soff
    return gpo, gpe, tgpe, np.float32(0.0)


def leaf_profile(code, subm, pen):
    """make_profile_n: the (len + 2) x 64 records of a sequence for the task with the penalties `pen` (task_penalties)"""
    out = np.zeros(64 * (len(code) + 2), np.float32)
    oracledrv.lib().ko_make_profile(_p(code), len(code), _p(subm), C.c_float(pen[0]), C.c_float(pen[1]), C.c_float(pen[2]), C.c_float(pen[3]), _p(out))
    return out


def task_operands(codes, subm, pen, a, b, nsip, plen, prof):
    """The two operands of task (a, b) as ko_msa_tree hands them to the DP and to the merge: a sequence's records made for this
    task, a node's merged profile with set_gap_penalties_n for the other side's member count.  prof[] is left as it is: a node's
    profile stays there AS CREATED."""
    L = oracledrv.lib()
    out = []
    for x, other in ((a, b), (b, a)):
        if nsip[x] == 1:
            out.append(leaf_profile(codes[x], subm, pen))
        else:
            p = np.array(prof[x], np.float32)
            L.ko_set_gap_penalties(_p(p), plen[x], nsip[other])
            out.append(p)
    return out


def merged_profile(pa, pb, coded, na, nb, subm, scal):
    """update_n along a coded path, with the unscaled penalties (aln_run.c:405-413): (coded[0] + 2) x 64 floats"""
    out = np.zeros(64 * (int(coded[0]) + 2), np.float32)
    coded = np.ascontiguousarray(coded, np.int32)
    oracledrv.lib().ko_update_profile(_p(pa), _p(pb), _p(out), _p(coded), na, nb, _p(subm),
                                      C.c_float(scal[0]), C.c_float(scal[1]), C.c_float(scal[2]), C.c_float(scal[5]))
    return out


class OracleExecutor:
    def __init__(self, codes, tasks, subm, scal, gap_scale, subm_off):
        """gap_scale / subm_off: per task, as do_align derives them (aln_run.c:226-237); taken from a
        whole-tree oracle run by the caller."""
        self.L = oracledrv.lib()
        self.codes = [np.ascontiguousarray(c, np.uint8) for c in codes]
        self.tasks = np.asarray(tasks)
        self.subm = np.ascontiguousarray(subm, np.float32).reshape(-1)
        self.scal = np.asarray(scal, np.float32)
        self.gap_scale, self.subm_off = gap_scale, subm_off
        n = len(codes)
        self.n = n
        self.plen = {i: len(c) for i, c in enumerate(codes)}
        self.nsip = {i: 1 for i in range(n)}
        for a, b, c in self.tasks:
            self.nsip[int(c)] = self.nsip[int(a)] + self.nsip[int(b)]
        self.prof = {}
        self.done = {}

    def tree_run_tasks(self, ids):
        for t in sorted(int(x) for x in ids):
            a, b, c = (int(v) for v in self.tasks[t])
            pen = task_penalties(self.scal, self.gap_scale[t], self.subm_off[t])
            gs = np.float32(self.gap_scale[t])
            gpo, gpe, tgpe, soff = pen
            la, lb = self.plen[a], self.plen[b]
            na, nb = self.nsip[a], self.nsip[b]
            pa, pb = task_operands(self.codes, self.subm, pen, a, b, self.nsip, self.plen, self.prof)
            swapped = 0
            if na == 1 and nb == 1:
                kind = 0
                if la < lb:
                    kw = dict(seq1=self.codes[a], seq2=self.codes[b])
                else:
                    swapped = 1
                    kw = dict(seq1=self.codes[b], seq2=self.codes[a])
                sip = 1
            elif na == 1:
                kind, swapped, sip = 1, 1, nb
                kw = dict(seq2=self.codes[a], prof1=pb)
            elif nb == 1:
                kind, sip = 1, na
                kw = dict(seq2=self.codes[b], prof1=pa)
            else:
                kind, sip = 2, 1
                if la < lb:
                    kw = dict(prof1=pa, prof2=pb)
                else:
                    swapped = 1
                    kw = dict(prof1=pb, prof2=pa)
            dla, dlb = (lb, la) if swapped else (la, lb)
            r = oracledrv.dp_single(kind, dla, dlb, self.subm, float(gpo), float(gpe), float(tgpe), float(soff), sip, **kw)
            raw = np.zeros(la + lb + 4, np.int32)
            raw[:dla + 2] = r["raw"]
            if swapped:
                raw2 = np.zeros(la + lb + 4, np.int32)
                self.L.ko_mirror_path(_p(raw), la, lb, _p(raw2))
                raw = raw2
            coded = np.zeros(la + lb + 3, np.int32)
            self.L.ko_code_path(_p(raw), la, lb, _p(coded))
            plen = int(coded[0])
            merged = np.zeros(64 * (plen + 2), np.float32)
            if t != len(self.tasks) - 1:
                merged = merged_profile(pa, pb, coded, na, nb, self.subm, self.scal)
            self.prof[c] = merged
            self.plen[c] = plen
            rec = oracledrv.TaskRec()
            rec.a, rec.b, rec.c = a, b, c
            rec.len_a, rec.len_b, rec.nsip_a, rec.nsip_b = la, lb, na, nb
            rec.plen, rec.kind, rec.swapped = plen, kind, swapped
            rec.meet, rec.transition, rec.score, rec.confidence = r["meet"], r["transition"], r["score"], r["confidence"]
            rec.gap_scale, rec.subm_off = float(gs), float(soff)
            self.done[t] = (rec, coded[:plen + 2].copy())

    def tree_get_node(self, node):
        return self.prof[node]

    def tree_set_node(self, node, prof):
        self.prof[node] = np.array(prof, np.float32)
        self.plen[node] = len(prof) // 64 - 2

    def tree_download_tasks(self, ids):
        recs, chunks, off = [], [], 0
        for t in ids:
            rec, path = self.done[int(t)]
            rec.path_off = off
            recs.append(rec)
            chunks.append(path)
            off += len(path)
        return recs, (np.concatenate(chunks) if chunks else np.zeros(0, np.int32))
