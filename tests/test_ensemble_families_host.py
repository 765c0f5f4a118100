"""The host side of the ensemble consensus stage for a batch of families (ka_ens_fam): the names and the ABI version,
ka_ens_fam_check on valid and broken packed batches (the family named, the one-family cause at the end), and the greedy
union, column order and fill through the seam ka_debug_ens_fam_consensus_host -- against the reference's consensus rows
stored in tests/golden/ens_*.npz, with the candidate lists restated in numpy from the stored members, and for any number
of threads.  No GPU: neither the check nor the seam needs a context."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

import poar_restate as pr
from util import GOLDEN

sys.path.insert(0, GOLDEN)

CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "ens_*.npz")))
FAMS = [["AC-D", "A-CD", "ACD-"], ["GGT-A", "G-TAA"], ["MK--L", "M-K-L", "MKL--", "--MKL"], ["W"], ["ST-", "-ST"]]
NAMES = ("ka_ens_fam_check", "ka_ens_fam_create", "ka_ens_fam_destroy", "ka_ens_fam_add_member", "ka_ens_fam_score_members",
         "ka_ens_fam_score", "ka_ens_fam_consensus", "ka_ens_fam_rows_size", "ka_ens_fam_rows", "ka_ens_fam_confidence",
         "ka_ens_fam_stats", "ka_debug_ens_fam_consensus_host")
WHY_4096 = "residue indices must stay below 4096 (the reference's POAR key ri << 20 | rj aliases beyond)"


def _check(L, fams, first=None, lens=None, widths=None):
    from kalign_amd import api
    rows, w = api.pack_families(fams)
    ff = api._fam_first([len(f) for f in fams]) if first is None else np.array(first, np.int32)
    ll = api.residue_lens([r for f in fams for r in f]) if lens is None else np.array(lens, np.int32)
    ww = w if widths is None else np.array(widths, np.int32)
    rc = L.ka_ens_fam_check(len(ff) - 1, api._ptr(ff), api._ptr(ll), api._ptr(rows), api._ptr(ww))
    return rc, L.ka_last_error().decode()


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, ensemble
    L = kalign_amd.load_library()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 19
    assert hasattr(kalign_amd.Context, "family_ensemble") and callable(ensemble.finish_ensembles)


def test_check_accepts_a_valid_batch():
    import kalign_amd
    L = kalign_amd.load_library()
    assert _check(L, FAMS)[0] == 0                                # (a family of one sequence among them, as ka_ens_create takes it)
    assert _check(L, [[r.lower().replace("-", ".") for r in f] for f in FAMS])[0] == 0


def test_check_refuses_fam_first():
    import kalign_amd
    L = kalign_amd.load_library()
    for first in ([1, 3, 5, 9, 10, 12], [0, 5, 3, 9, 10, 12]):
        rc, msg = _check(L, FAMS, first=first)
        assert rc != 0 and msg == "ka_ens_fam_check: fam_first does not ascend from 0 to numseq"
    rc, msg = _check(L, FAMS, first=[0, 3, 3, 9, 10, 12])
    assert rc != 0 and msg == "ka_ens_fam_check: empty family"


def test_check_refuses_a_letter_count_in_family_3_of_5():
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    fams = [FAMS[0], FAMS[1], FAMS[4], FAMS[2], FAMS[3]]
    lens = api.residue_lens([r for f in fams for r in f])
    lens[3 + 2 + 2 + 1] += 1                                      # family 3, its row 1
    rc, msg = _check(L, fams, lens=lens)
    assert rc != 0 and msg == ("ka_ens_fam_check: family 3: row 1 holds 3 letters, its sequence 4 "
                               "(every alignment must hold the same sequences)")


def test_check_refuses_a_sequence_of_4097_residues():
    import kalign_amd
    L = kalign_amd.load_library()
    long_ = "A" * 4097
    rc, msg = _check(L, [FAMS[0], ["ACGT" + "-" * 4093, long_]])
    assert rc != 0 and msg == "ka_ens_fam_check: family 1: sequence 1 has 4097 residues; " + WHY_4096
    assert _check(L, [FAMS[0], ["ACGT" + "-" * 4092, long_[1:]]])[0] == 0        # 4096 is the limit itself


def test_check_refuses_a_width():
    import kalign_amd
    L = kalign_amd.load_library()
    rc, msg = _check(L, FAMS, widths=[4, 0, 5, 1, 3])
    assert rc != 0 and msg == "ka_ens_fam_check: family 1: alignment width 0 does not fit row stride 1"
    rc, msg = _check(L, FAMS, widths=[4, 5, -1, 1, 3])            # (only ka_ens_fam_score skips a family)
    assert rc != 0 and msg == "ka_ens_fam_check: family 2: alignment width -1 does not fit row stride 0"


@pytest.mark.parametrize("n_runs", [0, 33])
def test_create_refuses_n_runs_before_the_context_is_used(n_runs):
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    first, lens = np.array([0, 2], np.int32), np.array([3, 4], np.int32)
    h = C.c_void_p()
    rc = L.ka_ens_fam_create(None, 1, api._ptr(first), api._ptr(lens), n_runs, C.byref(h))
    assert rc != 0 and not h.value
    assert L.ka_last_error().decode() == ("ka_ens_fam_create: n_runs %d outside 1..32 (one bit per member in the reference's POAR table)" % n_runs)
    # ... and the families, with the family named
    lens[1] = 4097
    rc = L.ka_ens_fam_create(None, 1, api._ptr(first), api._ptr(lens), 3, C.byref(h))
    assert rc != 0 and L.ka_last_error().decode() == "ka_ens_fam_create: family 0: sequence 1 has 4097 residues; " + WHY_4096


def candidates(members, lens, min_support):
    """build_consensus' candidate list restated from member rows: the POAR table's entries (pairs i < j ascending, keys
    ascending inside a pair) held by at least min_support members, support levels descending, inside a level in table
    order; as residue numbers flat inside the family: int32 [n, 2]"""
    n = len(lens)
    image = pr.poar_image(members)
    keys, masks = pr.entries(image, n)
    counts = pr.pair_counts(image, n).astype(np.int64)
    pi, pj = np.triu_indices(n, 1)                                # (pairs in the table's order)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    a = offs[np.repeat(pi, counts)] + (keys >> 20)
    b = offs[np.repeat(pj, counts)] + (keys & 0xFFFFF)
    level = pr.popcounts(masks) if len(masks) else np.zeros(0, np.int64)
    out = [np.zeros((0, 2), np.int64)]
    for L in range(len(members), min_support - 1, -1):
        pick = level == L
        out.append(np.stack([a[pick], b[pick]], axis=1))
    return np.concatenate(out).astype(np.int32)


def test_golden_cases_exist():
    assert len(CASES) >= 5, CASES


@pytest.fixture(scope="module")
def golden_batch():
    """every stored case at every stored min_support as one batch: (lengths, candidates, letters, the reference's rows)"""
    fam_lens, cands, letters, want = [], [], [], []
    for name in CASES:
        z, seqs, members, _ = pr.load_case(name)
        lens = [len(s) for s in seqs]
        for m in z["min_supports"]:
            fam_lens.append(lens)
            cands.append(candidates(members, lens, int(m)))
            letters.append(seqs)
            want.append([str(x).encode() for x in z["cons%d" % int(m)]])
    return fam_lens, cands, letters, want


@pytest.mark.parametrize("n_threads", [1, 4, 16])
def test_seam_against_the_golden_consensus_rows(golden_batch, n_threads):
    """the rows the reference built, for any number of threads"""
    from kalign_amd import api
    fam_lens, cands, letters, want = golden_batch
    got = api.ens_fam_consensus_host(fam_lens, cands, letters, n_threads)
    assert len(got) == len(want) >= 2 * len(CASES)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, f


def _random_batch():
    import make_golden_ensemble as mg
    rng = np.random.default_rng(40)
    fam_lens, cands, letters = [], [], []
    for f in range(40):
        seqs, members = mg.synthetic(int(rng.integers(2, 13)), int(rng.integers(10, 41)), int(rng.integers(1, 7)), 100 + f, moves=4)
        lens = [len(s) for s in seqs]
        fam_lens.append(lens)
        cands.append(candidates(members, lens, 1))
        letters.append(seqs)
    return fam_lens, cands, letters


def test_the_result_does_not_depend_on_the_threads():
    from kalign_amd import api
    fam_lens, cands, letters = _random_batch()
    one = api.ens_fam_consensus_host(fam_lens, cands, letters, 1)
    assert one == api.ens_fam_consensus_host(fam_lens, cands, letters, 16)
    for rows, seqs in zip(one, letters):                           # an alignment of the family's own sequences
        assert len({len(r) for r in rows}) == 1
        assert [r.replace(b"-", b"").decode() for r in rows] == seqs


def test_seam_refuses_what_it_cannot_replay():
    from kalign_amd import KalignAmdError, api
    with pytest.raises(KalignAmdError, match="family 1: a candidate names a residue outside the family"):
        api.ens_fam_consensus_host([[2, 2], [1, 2]], [[[0, 2]], [[0, 3]]], [["AC", "AG"], ["A", "AG"]], 2)
    with pytest.raises(KalignAmdError, match="n_threads 17 outside 1..16"):
        api.ens_fam_consensus_host([[2, 2]], [[[0, 2]]], [["AC", "AG"]], 17)
    rows, single = api.ens_fam_consensus_host([[2, 2], [1]], [[[0, 2]], []], [["AC", "AG"], ["W"]], 2)
    assert single == [b"W"] and len(rows[0]) == len(rows[1]) == 3 and rows[0][:1] == rows[1][:1] == b"A"
    assert [r.replace(b"-", b"") for r in rows] == [b"AC", b"AG"]
