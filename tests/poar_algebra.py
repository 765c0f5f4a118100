"""Merge and select of POAR tables restated on file images in numpy (the format: tests/poar_restate.py): what ka_ens_merge
and ka_ens_select must give.

    merge   per pair the sorted union of the two key lists; a key of both gets mask_a | mask_b << n_alignments(a), a key of
            b alone mask_b << n_alignments(a), a key of a alone mask_a; n_alignments = the sum
    select  new bit t of a mask = old bit members[t]; an entry whose new mask is 0 is dropped; keys and their order stay
"""
import numpy as np

from poar_restate import MAGIC


def split_image(image):
    """(numseq, n_alignments, [(keys, masks) of every pair in file order])"""
    w = np.frombuffer(image, np.uint32)
    assert int(w[0]) == MAGIC and int(w[1]) == 1
    n, r = int(w[2]), int(w[3])
    pairs, at = [], 4
    for _ in range(n * (n - 1) // 2):
        c = int(w[at])
        e = w[at + 1:at + 1 + 2 * c].reshape(c, 2)
        pairs.append((e[:, 0], e[:, 1]))
        at += 1 + 2 * c
    assert at == len(w)
    return n, r, pairs


def join_image(n, r, pairs):
    out = [np.array([MAGIC, 1, n, r], np.uint32).tobytes()]
    for keys, masks in pairs:
        e = np.empty((len(keys), 2), np.uint32)
        e[:, 0], e[:, 1] = keys, masks
        out += [np.uint32(len(keys)).tobytes(), e.tobytes()]
    return b"".join(out)


def merge_images(a, b):
    n, ra, pa = split_image(a)
    nb, rb, pb = split_image(b)
    assert n == nb and ra + rb <= 32
    out = []
    for (ka, ma), (kb, mb) in zip(pa, pb):
        keys = np.union1d(ka, kb)
        masks = np.zeros(len(keys), np.uint64)
        masks[np.searchsorted(keys, ka)] |= ma.astype(np.uint64)
        masks[np.searchsorted(keys, kb)] |= mb.astype(np.uint64) << np.uint64(ra)
        out.append((keys, masks.astype(np.uint32)))
    return join_image(n, ra + rb, out)


def select_image(image, members):
    n, r, pairs = split_image(image)
    members = [int(k) for k in members]
    assert 1 <= len(members) <= r and len(set(members)) == len(members) and all(0 <= k < r for k in members)
    out = []
    for keys, masks in pairs:
        new = np.zeros(len(keys), np.uint32)
        for t, k in enumerate(members):
            new |= ((masks >> np.uint32(k)) & np.uint32(1)) << np.uint32(t)
        out.append((keys[new != 0], new[new != 0]))
    return join_image(n, len(members), out)


def splits(r):
    """the split points of an R-member case: 1, R // 2, R - 1, and for 32 members also 16 and 31 (bit 31 arrives by shift)"""
    return sorted({1, r // 2, r - 1} | ({16, 31} if r == 32 else set()))
