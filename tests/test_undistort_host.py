"""compv_amd/csrc/undistort_math.hpp -- the arithmetic the undistortion kernels and host entry points are made of -- run on the host by
tests/host/undistort_math_check.cpp (a stand-alone program with its own main, standard library only, no GPU, built with AddressSanitizer and UBSan,
nothing preloaded) and held against tests/undistort_model.py and the fixture the compiled reference made, byte for byte: coefficient records, both map
planes in float32 and float64, the point cases, the projection cases with their z == 0 branch.  The program walks a map the way the kernels do (groups
of 4 entries, a partial group at the end of a row) and aborts when that differs from the plain walk."""
import struct
import subprocess

import numpy as np
import pytest

import undistort_cases as uc
import undistort_model as um
from fixtures import load_golden
from host_programs import ASAN_UBSAN_STATIC, WARN, build, host_cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("undistort_math_check.cpp", tmp_path_factory.mktemp("undistort"), host_cxx(), ["-O2", "-g", "-ffp-contract=off", *WARN, *ASAN_UBSAN_STATIC])

    def run(K, d, T, window=(0, 0, 0, 0), pts=None, pose=None, pts3=None):
        """-> None for a singular camera, else dict(coeffs, mx, my, pts, proj)"""
        folder = exe.parent
        x0, y0, wo, ho = window
        K, d = np.ascontiguousarray(K, T), np.ascontiguousarray(d, T).ravel()
        pts = np.zeros((0, 2), T) if pts is None else np.ascontiguousarray(pts, T)
        nproj = 0 if pts3 is None else len(pts3)
        with open(folder / "in.bin", "wb") as f:
            f.write(struct.pack("<8i", int(T is np.float64), d.size, x0, y0, wo, ho, len(pts), nproj))
            f.write(K.tobytes() + d.tobytes() + pts.tobytes())
            if nproj:
                f.write(np.ascontiguousarray(pose, np.float64).tobytes() + np.ascontiguousarray(pts3, np.float64).tobytes())
        r = subprocess.run([str(exe), str(folder / "in.bin"), str(folder / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = open(folder / "out.bin", "rb").read()
        if struct.unpack_from("<i", raw)[0] == 0:
            assert len(raw) == 4
            return None
        item = np.dtype(T).itemsize
        body = np.frombuffer(raw, T, (len(raw) - 4 - nproj * 16) // item, 4)
        n = wo * ho
        assert body.size == 14 + 2 * n + 2 * len(pts)
        return {"coeffs": body[:14], "mx": body[14:14 + n].reshape(ho, wo), "my": body[14 + n:14 + 2 * n].reshape(ho, wo), "pts": body[14 + 2 * n:].reshape(-1, 2),
                "proj": np.frombuffer(raw, np.float64, 2 * nproj, len(raw) - nproj * 16).reshape(-1, 2)}
    return run


@pytest.fixture(scope="module")
def arrays():
    return load_golden("golden_undistort")[1]


@pytest.mark.parametrize("c", uc.image_cases(), ids=lambda c: c["id"])
def test_coefficients_and_maps(checker, arrays, c):
    wo, ho = c["size"][2:]
    for T in (np.float32, np.float64):
        got = checker(c["K"], c["d"], T, (*c["origin"], wo, ho))
        assert got["coeffs"].tobytes() == um.coeffs(c["K"], c["d"], T).tobytes()
        mx, my = um.map_planes(c["K"], c["d"], wo, ho, *c["origin"], dtype=T)
        assert got["mx"].tobytes() == mx.tobytes() and got["my"].tobytes() == my.tobytes()
        if T is np.float32:
            assert got["mx"].tobytes() == arrays["mapx_" + c["id"]].tobytes() and got["my"].tobytes() == arrays["mapy_" + c["id"]].tobytes()


@pytest.mark.parametrize("c", uc.point_cases(), ids=lambda c: c["id"])
def test_points(checker, arrays, c):
    cam = uc.case(c["camera"])
    got = checker(cam["K"], cam["d"], c["dtype"], pts=uc.points(c))
    assert got["pts"].tobytes() == arrays[c["id"]].tobytes() == um.dist_points(cam["K"], cam["d"], uc.points(c), c["dtype"]).tobytes()


@pytest.mark.parametrize("c", uc.proj_cases(), ids=lambda c: c["id"])
def test_projection(checker, arrays, c):
    cam = uc.case(c["camera"])
    pose = np.concatenate([np.asarray(c["R"], np.float64).ravel(), np.asarray(c["t"], np.float64)])
    got = checker(cam["K"], cam["d"], np.float64, pose=pose, pts3=uc.proj_points(c))
    assert got["proj"].tobytes() == arrays[c["id"]].tobytes()


def test_refusals(checker):
    K = uc.case("pin61")["K"]
    assert checker(K, (0.1,), np.float32) is None and checker(K, (0.1, 0.2, 0.3, 0.4, 0.5), np.float64) is None          # nd outside 2 .. 4
    singular = [[0.0, 0.0, 3.0], [0.0, 5.0, 2.0], [0.0, 0.0, 1.0]]
    assert checker(singular, (0.1, 0.2), np.float32) is None and checker(singular, (0.1, 0.2), np.float64) is None
