"""The POAR file (poar_table_write, lib/src/poar.c:203-252) restated from member rows alone, in numpy: what
tests/golden/poar_*.npz pin and what the device's table pass must write.

    "POAR" (u32 0x524F4150, little endian) | u32 version = 1 | u32 numseq | u32 n_alignments
    for every pair i < j (i ascending, then j):
        u32 n_entries | n_entries x { u32 key = ri << 20 | rj ; u32 mask (bit k: member k aligns ri with rj) }, keys ascending
"""
import hashlib
import os

import numpy as np

MAGIC = 0x524F4150
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def position_maps(rows):
    """per row: the residue index at every column, -1 at gaps (a residue is an ASCII letter)"""
    out = []
    for r in rows:
        a = np.frombuffer(r.encode() if isinstance(r, str) else bytes(r), np.uint8) | 32
        isres = (a >= 97) & (a <= 122)
        out.append(np.where(isres, np.cumsum(isres) - 1, -1))
    return out


def poar_image(members):
    """members[k][s]: row s of member k (str / bytes); the file's bytes"""
    n = len(members[0])
    maps = [position_maps(rows) for rows in members]
    out = [np.array([MAGIC, 1, n, len(members)], np.uint32).tobytes()]
    for i in range(n - 1):
        for j in range(i + 1, n):
            d = {}
            for k, m in enumerate(maps):
                both = (m[i] >= 0) & (m[j] >= 0)
                keys = (m[i][both].astype(np.uint32) << 20) | m[j][both].astype(np.uint32)
                for key in keys.tolist():
                    d[key] = d.get(key, 0) | (1 << k)
            ks = sorted(d)
            e = np.empty((len(ks), 2), np.uint32)
            e[:, 0], e[:, 1] = ks, [d[x] for x in ks]
            out += [np.uint32(len(ks)).tobytes(), e.tobytes()]
    return b"".join(out)


def pair_counts(image, n):
    """n_entries of every pair of a well-formed image, in file order (uint32[n * (n - 1) / 2])"""
    w = np.frombuffer(image, np.uint32)
    out = np.zeros(n * (n - 1) // 2, np.uint32)
    at = 4
    for p in range(len(out)):
        out[p] = w[at]
        at += 1 + 2 * int(w[at])
    assert at == len(w), "the image is longer or shorter than its counts imply"
    return out


def pair_offsets(image, n):
    """byte offset of every pair's count word"""
    c = pair_counts(image, n).astype(np.int64)
    return 16 + np.concatenate([[0], np.cumsum(4 + 8 * c)[:-1]]) if len(c) else np.zeros(0, np.int64)


def entries(image, n):
    """(keys, masks) of all entries in file order"""
    w = np.frombuffer(image, np.uint32)[4:]
    keep = np.ones(len(w), bool)
    keep[(pair_offsets(image, n) - 16) // 4] = False
    e = w[keep].reshape(-1, 2)
    return e[:, 0], e[:, 1]


def popcounts(masks):
    return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


def sha256(image):
    return hashlib.sha256(image).hexdigest()


def load_case(name):
    """(ens_<name>.npz, seqs, members, poar_<name>.npz)"""
    z = np.load(os.path.join(GOLDEN, "ens_%s.npz" % name))
    seqs = [str(s) for s in z["seqs"]]
    members = [["".join(r) for r in m] for m in z["members"]]
    return z, seqs, members, np.load(os.path.join(GOLDEN, "poar_%s.npz" % name))
