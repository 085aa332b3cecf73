"""compv_amd/csrc/moments_math.hpp -- the range rule and the shape record the moments kernels and host entry points are made of -- run on the host by
tests/host/moments_math_check.cpp (a stand-alone program with its own main, standard library only, no GPU, built with AddressSanitizer and UBSan, nothing
preloaded) and held against tests/moments_model.py on every byte of every record of the fixture, and against the reference's skew and theta."""
import struct
import subprocess

import numpy as np
import pytest

import moments_model as mm
from fixtures import load_golden
from host_programs import ASAN_UBSAN_STATIC, WARN, build, host_cxx

SHAPE_DTYPE = np.dtype([(k, "<f8") for k in mm.SHAPE_NAMES] + [("status", "<i4"), ("pad", "<i4")])
SIZES = [(3840, 2160, mm.VALUE), (16384, 16384, mm.VALUE), (32767, 32767, mm.VALUE), (32767, 32767, mm.UNIT), (1, 1, mm.VALUE), (0, 4, mm.UNIT), (4, 0, mm.UNIT),
         (32768, 1, mm.UNIT), (1, 32768, mm.UNIT), (65536, 32767, mm.UNIT), (5, 5, 2), (5, 5, -1), (16406, 16384, mm.VALUE), (16407, 16384, mm.VALUE), (32767, 2056, mm.VALUE),
         (2057, 32767, mm.VALUE), (32767, 1, mm.VALUE), (1, 32767, mm.VALUE)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("moments_math_check.cpp", tmp_path_factory.mktemp("moments"), host_cxx(), ["-O2", "-g", "-ffp-contract=off", *WARN, *ASAN_UBSAN_STATIC])

    def run(raw, sizes=()):
        folder = exe.parent
        raw = np.ascontiguousarray(raw, np.uint64).reshape(-1, 6)
        with open(folder / "in.bin", "wb") as f:
            f.write(struct.pack("<2i", len(raw), len(sizes)) + raw.tobytes() + np.array(sizes, np.int32).tobytes())
        r = subprocess.run([str(exe), str(folder / "in.bin"), str(folder / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = open(folder / "out.bin", "rb").read()
        assert len(out) == 72 * len(raw) + 4 * len(sizes)
        return np.frombuffer(out, SHAPE_DTYPE, len(raw)), np.frombuffer(out, np.int32, len(sizes), 72 * len(raw)).tolist()
    return run


def test_shape_records_of_the_fixture(checker):
    meta, arrays = load_golden("golden_moments")
    names = [k for k in arrays.files if k.startswith("raw_")]
    raw = np.concatenate([arrays[k].reshape(-1, 6) for k in names])
    assert len(raw) > 150
    got, _ = checker(raw)
    assert got.tobytes() == mm.shape_array([tuple(int(v) for v in r) for r in raw], SHAPE_DTYPE).tobytes()
    # against the reference itself: skew on every bit, theta within the bound
    row = 0
    frames = {r["id"]: r for r in meta["frames"]}
    for k in names:
        n = arrays[k].reshape(-1, 6).shape[0]
        rec = frames.get(k[4:])
        if rec is None:
            skews, thetas = arrays["skew_" + k[4:]], arrays["theta_" + k[4:]]
        elif rec.get("model_only"):
            row += n
            continue
        else:
            skews, thetas = [float.fromhex(rec["skew"])], [float.fromhex(rec["theta"])]
        for i in range(n):
            g = got[row + i]
            assert np.float64(g["skew"]).tobytes() == np.float64(skews[i]).tobytes(), (k, i)
            if mm.angle_case({name: g[name] for name in SHAPE_DTYPE.names}):
                assert abs(np.arctan2(g["sn"], g["cs"]) - thetas[i]) <= 4 * meta["max_angle_distance"], (k, i)
        row += n
    assert row == len(raw)


def test_records_at_the_edges(checker):
    """an empty record, sums at and around 2^53 and 2^64 - 1 (the conversion rounds to nearest even), a den of exactly 0"""
    raw = [(0, 0, 0, 0, 0, 0), (0, 5, 5, 5, 5, 5), (1, 0, 0, 0, 0, 0), (10, 20, 30, 70, 50, 100), (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 64 - 1, 2 ** 63 + 1025, 2 ** 64 - 1025),
           (3, 2 ** 40, 2 ** 41 + 1, 2 ** 62, 2 ** 63, 2 ** 64 - 1)]
    got, _ = checker(raw)
    assert got.tobytes() == mm.shape_array(raw, SHAPE_DTYPE).tobytes()
    assert got[0]["status"] == 1 and got[1]["status"] == 1 and got[2]["status"] == 0 and (got[3]["cs"], got[3]["sn"], got[3]["skew"]) == (1.0, 0.0, 1.0)


def test_the_range_rule(checker):
    _, fits = checker(np.zeros((0, 6), np.uint64), SIZES)
    assert fits == [int(mm.fits(w, h, k)) for w, h, k in SIZES]
    assert fits[:4] == [1, 1, 0, 1] and fits[12:16] == [1, 0, 1, 0]          # both sides of 2^64
