"""The ensemble consensus stage restated from a POAR table (tests/poar_restate.py) in numpy: what ka_ens and ka_ens_fam must
give for an alignment X of the table's sequences, with the expressions of DESIGN 4k.

    support(i, ri, j, rj)   popcount of the mask of key ri << 20 | rj in pair (i, j), i < j; 0 when no member holds it
    score sum               sum over X's aligned pairs of (support - 1): an exact integer
    residue confidence      (float)(sum of support over the residue's partners / ((double)partners * n_runs)), 0 at gaps
    column confidence       the column's residue confidences added in row order in double, (float)(sum / count)
    candidates              levels n_runs .. min_support, inside a level the table's order: (flat residue of i, flat residue of j)
    consensus rows          those candidates through the library's host-only greedy union (ka_debug_ens_fam_consensus_host)
"""
import numpy as np

import poar_restate as pr


class Table:
    def __init__(self, image, lens):
        head = np.frombuffer(image[:16], np.uint32)
        self.n, self.runs = int(head[2]), int(head[3])
        self.lens = [int(x) for x in lens]
        assert len(self.lens) == self.n
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.keys, masks = pr.entries(image, self.n)
        self.sup = pr.popcounts(masks).astype(np.int64)
        counts = pr.pair_counts(image, self.n).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(counts)])
        self.pair_of = np.repeat(np.arange(len(counts)), counts)
        ii, jj = np.triu_indices(self.n, 1)                      # (the file's pair order: i ascending, then j)
        self.pi, self.pj = ii.astype(np.int64), jj.astype(np.int64)

    @classmethod
    def of_members(cls, members, lens):
        return cls(pr.poar_image(members), lens)

    def pair(self, i, j):
        return i * self.n - i * (i + 1) // 2 + (j - i - 1)

    def support(self, i, j, ri, rj):
        """support of the residue pairs (ri[x] of i, rj[x] of j), i < j"""
        p = self.pair(i, j)
        keys = self.keys[self.start[p]:self.start[p + 1]]
        want = (ri.astype(np.uint32) << 20) | rj.astype(np.uint32)
        at = np.searchsorted(keys, want)
        hit = at < len(keys)
        hit[hit] = keys[at[hit]] == want[hit]
        out = np.zeros(len(want), np.int64)
        out[hit] = self.sup[self.start[p] + at[hit]]
        return out

    def _walk(self, rows):
        """per pair i < j of X: (i, j, ri, rj, support) of its aligned residue pairs"""
        m = pr.position_maps(rows)
        for i in range(self.n - 1):
            for j in range(i + 1, self.n):
                both = (m[i] >= 0) & (m[j] >= 0)
                ri, rj = m[i][both], m[j][both]
                yield i, j, ri, rj, self.support(i, j, ri, rj)

    def score(self, rows):
        """(the exact sum, score_alignment_poar's double)"""
        s = sum(int((sup - 1).sum()) for _, _, _, _, sup in self._walk(rows))
        return s, s / (self.runs - 1 if self.runs > 1 else 1.0)

    def confidence(self, rows):
        """(float32[n, width], float32[width])"""
        m = pr.position_maps(rows)
        width = len(m[0]) if m else 0
        tot = [np.zeros(n, np.int64) for n in self.lens]
        cnt = [np.zeros(n, np.int64) for n in self.lens]
        for i, j, ri, rj, sup in self._walk(rows):
            np.add.at(tot[i], ri, sup); np.add.at(cnt[i], ri, 1)
            np.add.at(tot[j], rj, sup); np.add.at(cnt[j], rj, 1)
        res = np.zeros((self.n, width), np.float32)
        for s in range(self.n):
            isres = m[s] >= 0
            r = m[s][isres]
            ok = cnt[s][r] > 0
            v = np.zeros(len(r), np.float32)
            v[ok] = (tot[s][r][ok].astype(np.float64) / (cnt[s][r][ok].astype(np.float64) * float(self.runs))).astype(np.float32)
            res[s, isres] = v
        acc = np.zeros(width, np.float64)
        num = np.zeros(width, np.int64)
        for s in range(self.n):                                  # row order, in double
            isres = m[s] >= 0
            acc[isres] += res[s, isres].astype(np.float64)
            num[isres] += 1
        col = np.zeros(width, np.float32)
        col[num > 0] = (acc[num > 0] / num[num > 0]).astype(np.float32)
        return res, col

    def candidates(self, min_support):
        """int32[n, 2]: levels n_runs .. max(min_support, 1), the table's order inside a level"""
        out = []
        for level in range(self.runs, max(int(min_support), 1) - 1, -1):
            e = np.flatnonzero(self.sup == level)
            p = self.pair_of[e]
            k = self.keys[e].astype(np.int64)
            out.append(np.stack([self.offs[self.pi[p]] + (k >> 20), self.offs[self.pj[p]] + (k & 0xFFFFF)], axis=1))
        return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 2), np.int32)

    def consensus(self, seqs, min_support):
        """the consensus rows (bytes) at min_support"""
        from kalign_amd import api
        return api.ens_fam_consensus_host([self.lens], [self.candidates(min_support)], [seqs])[0]
