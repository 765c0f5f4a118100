"""Writes tests/golden/idm_*.npz: python-kalign's kalign.utils.pairwise_identity_matrix run on the rows of every stored
tests/golden/sum_*.npz case.  Needs the reference's sources and no GPU:

    python tests/golden/make_golden_identity.py [REFERENCE_ROOT]        (default: $KALIGN_REF or /root/reference)

utils.py is loaded by path (the package itself needs its compiled extension).  idm_<case>.npz holds data only:
    identity     float64 [n, n]: the utility's matrix for the `rows` of sum_<case>.npz (the utility gets them as str, a byte
                 as the latin-1 character)
The rows are not stored again: a test reads them from the sum_ file of the same name.
"""
import glob
import os
import sys

import numpy as np

from make_golden_summary import HERE, load_utils


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KALIGN_REF", "/root/reference")
    u = load_utils(root)
    for src in sorted(glob.glob(os.path.join(HERE, "sum_*.npz"))):
        name = os.path.basename(src)[4:-4]
        a = np.load(src)["rows"]
        ident = np.asarray(u.pairwise_identity_matrix([bytes(r).decode("latin-1") for r in a]), np.float64)
        assert ident.shape == (a.shape[0], a.shape[0])
        path = os.path.join(HERE, "idm_%s.npz" % name)
        np.savez_compressed(path, identity=ident)
        assert os.path.getsize(path) < 100 * 1000, (name, os.path.getsize(path))
        print("%-28s %3d x %4d  %6d bytes" % (name, a.shape[0], a.shape[1], os.path.getsize(path)))


if __name__ == "__main__":
    main()
