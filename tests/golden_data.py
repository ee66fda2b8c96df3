"""Loader of the golden fixtures under tests/golden/.  A fixture too large for one file (every committed file stays under 1 MiB) is
stored in parts: golden_<name>.npz plus golden_<name>_<column>.npz (written so by tests/golden/make_fixtures.py)."""
import glob
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    """The arrays of fixture `name` (e.g. "res2") as one dict, parts joined."""
    d = dict(np.load(os.path.join(G, "golden_%s.npz" % name)))
    for part in sorted(glob.glob(os.path.join(G, "golden_%s_*.npz" % name))):
        d.update(np.load(part))
    return d
