"""CPU: the algebra on POAR tables (ka_ens_merge / ka_ens_select) without a GPU -- the entry points are there, and the numpy
statement of merge and select on file images (tests/poar_algebra.py), the oracle's companion in test_gpu_poar_merge.py,
reproduces the stored image or SHA-256 of every tests/golden/poar_*.npz case from a split of its members."""
import glob
import os

import numpy as np
import pytest

import poar_algebra
import poar_restate
from util import GOLDEN

CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "poar_*.npz")))


def test_names_and_abi_version():
    from kalign_amd import api, ensemble
    L = api.load_library()
    assert L.ka_abi_version() >= 14
    for name in ("ka_ens_merge", "ka_ens_select"):
        assert name in api.EXPORTS and hasattr(L, name), name
    assert callable(api.Ensemble.merge) and callable(api.Ensemble.select)
    assert callable(ensemble.extend_poar)


@pytest.mark.parametrize("name", CASES)
def test_merged_split_is_the_stored_table(name):
    """one image per member, folded with merge_images on either side of every split point: the case's stored bytes"""
    z, seqs, members, want = poar_restate.load_case(name)
    one = [poar_restate.poar_image([m]) for m in members]

    def fold(images):
        out = images[0]
        for x in images[1:]:
            out = poar_algebra.merge_images(out, x)
        return out
    for s in poar_algebra.splits(len(members)):
        image = poar_algebra.merge_images(fold(one[:s]), fold(one[s:]))
        assert len(image) == int(want["size"]) and poar_restate.sha256(image) == str(want["sha256"]), s
        if "image" in want.files:
            assert image == want["image"].tobytes(), s


def test_r3_members_are_the_first_three_of_r8():
    for case in ("real_bb11001", "real_bb30014", "real_dna40"):
        z3, seqs3, m3, w3 = poar_restate.load_case(case + "_r3")
        z8, seqs8, m8, w8 = poar_restate.load_case(case + "_r8")
        assert seqs3 == seqs8 and m3 == m8[:3] and len(m8) == 8, case


@pytest.mark.parametrize("name,sel", [("syn8", [0]), ("syn8", [7]), ("syn8", list(range(1, 8))), ("syn8", list(range(7, -1, -1))),
                                      ("syn32", [31, 0]), ("syn3", [2, 0])])
def test_select_is_the_table_of_those_members(name, sel):
    z, seqs, members, want = poar_restate.load_case(name)
    assert poar_algebra.select_image(want["image"].tobytes(), sel) == poar_restate.poar_image([members[k] for k in sel])


def test_select_identity_and_split_merge_round_trip():
    z, seqs, members, want = poar_restate.load_case("syn8dna")
    image = want["image"].tobytes()
    assert poar_algebra.select_image(image, range(8)) == image
    for s in (1, 4, 7):
        assert poar_algebra.merge_images(poar_algebra.select_image(image, range(s)), poar_algebra.select_image(image, range(s, 8))) == image


def test_order_matters():
    z, seqs, members, want = poar_restate.load_case("syn3")
    a, b = poar_restate.poar_image(members[:1]), poar_restate.poar_image(members[1:])
    assert poar_algebra.merge_images(b, a) == poar_restate.poar_image(members[1:] + members[:1])
    assert poar_algebra.merge_images(b, a) != poar_algebra.merge_images(a, b) == want["image"].tobytes()
