"""Oracle vs the compiled reference for the optional Gaussian pre-blur:
CompVMathGauss::kernelDim1 / kernelDim1FixedPoint and CompVMathConvlt::convlt1FixedPoint, incl. the reference's own
known-answer vector unittests/math_convlt.cxx:21 (case 0, MD5 2678b73a89681f12fb474dd8102fc37c)."""
import numpy as np
import pytest

from gauss_cases import CASE0_KERNEL_LITERAL, case0_input
from oracle_bindings import md5_rows


def test_case0_kernel_bytes_match_reference(refshim):
    k = refshim.gauss_kernel_f32(7, 3.5)
    assert k.view(np.uint16).tolist() == CASE0_KERNEL_LITERAL


def test_reference_known_answer_case0(oracle):
    """The reference's own golden for the fixed-point convolution (kernel = 7 of the u16 halves above, both passes)."""
    kern = np.array(CASE0_KERNEL_LITERAL[:7], np.uint16)
    rc, out = oracle.convlt_fxp(case0_input(), kern, kern)
    assert rc == 0 and md5_rows(out) == "2678b73a89681f12fb474dd8102fc37c"


@pytest.mark.parametrize("size,sigma", [(3, 0.8), (5, 1.0), (5, 1.4), (7, 2.0), (7, 3.5), (9, 2.5), (15, 4.0)])
def test_gauss_kernels_match_reference(oracle, refshim, size, sigma):
    assert oracle.gauss_kernel_f32(size, sigma).view(np.uint32).tolist() == refshim.gauss_kernel_f32(size, sigma).view(np.uint32).tolist()
    assert oracle.gauss_kernel_fxp(size, sigma).tolist() == refshim.gauss_kernel_fxp(size, sigma).tolist()


@pytest.mark.parametrize("W,H,S", [(64, 16, 64), (333, 77, 384), (641, 48, 704), (1282, 40, 1344)])
@pytest.mark.parametrize("size", [3, 5, 7, 9, 15])
def test_convlt_fixedpoint_matches_reference(oracle, refshim, W, H, S, size):
    rng = np.random.default_rng(W * 31 + size)
    img = np.zeros((H, S), np.uint8)
    img[:, :W] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img = img[:, :W]
    for kern in (oracle.gauss_kernel_fxp(size, 0.3 * size), rng.integers(0, 65536 // size, size).astype(np.uint16),
                 np.full(size, 65535, np.uint16)):                          # the last one saturates every pixel
        vt = kern
        hz = kern[::-1].copy() if size > 3 else kern
        rc0, exp = refshim.convlt_fxp(img, vt, hz)
        rc1, got = oracle.convlt_fxp(img, vt, hz)
        assert rc0 == 0 and rc1 == 0
        assert (got == exp).all(), int((got != exp).sum())


def test_convlt_fixedpoint_rejects_bad_geometry(oracle):
    img = np.zeros((4, 16), np.uint8)
    rc, _ = oracle.convlt_fxp(img, [1, 2, 3, 2, 1], [1, 2, 3, 2, 1])            # H < k (compv_math_convlt.h:100)
    assert rc != 0
    rc, _ = oracle.convlt_fxp(np.zeros((16, 16), np.uint8), [1, 2, 3, 4], [1, 2, 3, 4])   # even size
    assert rc != 0


@pytest.mark.parametrize("size,sigma", [(3, 0.8), (5, 1.0), (7, 2.0), (7, 3.5), (9, 2.5), (15, 4.0)])
def test_capi_gauss_kernel_host_logic(oracle, size, sigma):
    """compvhip_gauss_kernel_fixedpoint is host arithmetic in the C-ABI library: it must equal the oracle's restatement."""
    from compv_amd import capi
    assert capi.gauss_kernel_fixedpoint(size, sigma).tolist() == oracle.gauss_kernel_fxp(size, sigma).tolist()
    with pytest.raises(capi.CompvHipError):
        capi.gauss_kernel_fixedpoint(4, 1.0)
