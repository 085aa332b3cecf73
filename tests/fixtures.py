"""The fixtures under tests/golden and the digest they are compared by, for CPU and GPU tests alike."""
import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden(stem):
    """(the JSON of tests/golden/<stem>.json, the arrays of <stem>.npz or None where the fixture has none)"""
    with open(os.path.join(GOLDEN_DIR, stem + ".json")) as f:
        meta = json.load(f)
    npz = os.path.join(GOLDEN_DIR, stem + ".npz")
    return meta, np.load(npz) if os.path.exists(npz) else None
