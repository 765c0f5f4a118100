"""CPU: the ensemble's POAR file (poar_table_write / poar_table_read, lib/src/poar.c:203-325) without a GPU -- the stored
fixtures (tests/golden/poar_*.npz, make_golden_poar.py) are what the format says (tests/poar_restate.py), and the reader's
checks (ka_poar_check_image, api.check_table) accept them and reject every kind of damaged file with its cause."""
import glob
import os

import numpy as np
import pytest

import poar_restate
from util import GOLDEN

CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "poar_*.npz")))
STORED = ["real_bb11001_r3", "real_bb11001_r8", "syn2", "syn3", "syn32", "syn8", "syn8dna"]      # cases with the image itself


def test_eleven_cases_one_per_ensemble_case():
    ens = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "ens_*.npz")))
    assert len(CASES) == 11 and CASES == ens
    assert [c for c in CASES if "image" in np.load(os.path.join(GOLDEN, "poar_%s.npz" % c)).files] == STORED


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_the_restatement_of_the_stored_members(name):
    z, seqs, members, want = poar_restate.load_case(name)
    image = poar_restate.poar_image(members)
    assert len(image) == int(want["size"])
    assert poar_restate.sha256(image) == str(want["sha256"])
    counts = poar_restate.pair_counts(image, len(seqs))
    assert counts.dtype == want["n_entries"].dtype == np.uint32 and np.array_equal(counts, want["n_entries"])
    assert len(image) == 16 + 4 * len(counts) + 8 * int(counts.sum())
    if "image" in want.files:
        assert want["image"].tobytes() == image


@pytest.mark.parametrize("name", STORED)
def test_check_table_accepts_the_stored_image(name, tmp_path):
    from kalign_amd import api
    z, seqs, members, want = poar_restate.load_case(name)
    image = want["image"].tobytes()
    lens = [len(s) for s in seqs]
    assert api.check_table(image, lens) == (len(members), int(want["n_entries"].sum()))
    p = tmp_path / "t.poar"
    p.write_bytes(image)
    assert api.check_table(str(p), lens) == (len(members), int(want["n_entries"].sum()))


def _syn8():
    z, seqs, members, want = poar_restate.load_case("syn8")
    return np.frombuffer(want["image"].tobytes(), np.uint32).copy(), [len(s) for s in seqs], want


def _first_pair_with(want, n, at_least):
    """(pair index, i, j) of the first pair holding at_least entries"""
    p = 0
    for i in range(n - 1):
        for j in range(i + 1, n):
            if want["n_entries"][p] >= at_least:
                return p, i, j
            p += 1
    raise AssertionError("no such pair")


def _damaged():
    """(name, bytes, lens, message pattern): one image per error of the reader, each a stored image with one change"""
    w, lens, want = _syn8()
    n = len(lens)
    good = w.tobytes()
    p, i, j = _first_pair_with(want, n, 3)
    e0 = int(poar_restate.pair_offsets(good, n)[p]) // 4 + 1          # word index of the pair's first key
    out = []

    def patch(name, pattern, **words):
        x = w.copy()
        for k, v in words.items():
            x[int(k[1:])] = v
        out.append((name, x.tobytes(), lens, pattern))
    patch("magic", "wrong magic", _0=0x524F4151)
    patch("version", "version 2 not supported", _1=2)
    patch("numseq", "numseq %d in the file, %d sequences given" % (n + 1, n), _2=n + 1)
    patch("n_alignments 0", "n_alignments 0 outside 1..32", _3=0)
    patch("n_alignments 33", "n_alignments 33 outside 1..32", _3=33)
    out.append(("one byte short", good[:-1], lens, "truncated"))
    out.append(("one byte long", good + b"\0", lens, "1 bytes after the last pair"))
    patch("ri = lens[i]", r"pair \(%d, %d\) entry 0: residue ri = %d but sequence %d has %d" % (i, j, lens[i], i, lens[i]),
          **{"_%d" % e0: (lens[i] << 20) | (int(w[e0]) & 0xFFFFF)})
    last = e0 + 2 * (int(want["n_entries"][p]) - 1)                     # the pair's last key: raising it keeps the order
    patch("rj = lens[j]", r"residue rj = %d but sequence %d has %d" % (lens[j], j, lens[j]),
          **{"_%d" % last: (int(w[last]) >> 20 << 20) | lens[j]})
    patch("two keys swapped", "entry 1: keys not strictly ascending", **{"_%d" % e0: w[e0 + 2], "_%d" % (e0 + 2): w[e0]})
    patch("a key twice", "entry 2: keys not strictly ascending", **{"_%d" % (e0 + 4): w[e0 + 2]})
    patch("mask 0", "entry 1: mask 0", **{"_%d" % (e0 + 3): 0})
    patch("a bit at n_alignments", "entry 0: mask 0x00000101 has a bit at or above n_alignments = 8", **{"_%d" % (e0 + 1): 0x101})
    return out


DAMAGED = _damaged() if "syn8" in CASES else []


def test_every_error_of_the_reader_has_a_case():
    assert len(DAMAGED) == 13


@pytest.mark.parametrize("case", DAMAGED, ids=[d[0] for d in DAMAGED])
def test_check_table_rejects(case):
    from kalign_amd import KalignAmdError, api
    name, image, lens, pattern = case
    with pytest.raises(KalignAmdError, match=pattern):
        api.check_table(image, lens)


def test_bit_31_is_a_member_like_any_other():
    from kalign_amd import api
    z, seqs, members, want = poar_restate.load_case("syn32")
    image = want["image"].tobytes()
    keys, masks = poar_restate.entries(image, len(seqs))
    assert len(keys) == int(want["n_entries"].sum()) and (masks >> 31).any()
    assert int(poar_restate.popcounts(masks).max()) == 32
    assert api.check_table(image, [len(s) for s in seqs])[0] == 32


def test_an_empty_image_is_a_truncated_file():
    from kalign_amd import KalignAmdError, api
    with pytest.raises(KalignAmdError, match="0 bytes, shorter than the 16-byte header"):
        api.check_table(b"", [3, 4])


def test_one_sequence_is_the_header_alone():
    from kalign_amd import api
    image = poar_restate.poar_image([["ACD"], ["AC-D"]])
    assert len(image) == 16 and api.check_table(image, [3]) == (2, 0)


def test_names_and_abi_version():
    from kalign_amd import api, ensemble
    L = api.load_library()
    assert L.ka_abi_version() >= 13
    for name in ("ka_ens_table_size", "ka_ens_table_write", "ka_ens_table_image", "ka_ens_open_table", "ka_ens_open_table_image",
                 "ka_ens_n_runs", "ka_ens_table_stats", "ka_poar_check_image"):
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("table_size", "write_table", "table_image"):
        assert callable(getattr(api.Ensemble, name))
    assert callable(api.Context.ensemble_from_table) and callable(api.check_table)
    assert callable(ensemble.consensus_from_poar)
    import inspect
    assert "save_poar_path" in inspect.signature(ensemble.finish_ensemble).parameters
