"""CPU tests of the canonical KHT order (COMPVHIP_KHT_ORDER_CANONICAL, include/compv_hip.h) and of its C ABI.

The model (tests/kht_canon_model.py) restates the reference's peak emission in numpy; its records must be exactly the oracle's, and the local line rule
the GPU applies per record must pick the same lines, in the same order, as the reference's sequential visited-map sweep run on the stably sorted list."""
import ctypes as C

import numpy as np
import pytest

from kht_canon_model import Axes, CanonModel, canonical, emission, local_lines, scan
from oracle_bindings import synth_frame

# the synthetic sizes of test_kht.py (+ a dense 1282 x 720 frame: rhoN % 4 == 3, records of the scalar remainder)
SIZES = [(640, 480, 59., 119., 1.0, 1.0, 1), (640, 480, 59., 119., 0.5, 1.0, 1), (480, 360, 59., 119., 1.0, 0.5, 150),
         (257, 129, 0.8, 1.6, 1.0, 2.0, 1), (97, 64, 20., 60., 1.0, 1.0, 1), (1282, 720, 0.8, 1.6, 1.0, 1.0, 1)]


@pytest.fixture(scope="module")
def model(oracle):
    return CanonModel(oracle)


def _records_as_lines(rec):
    return [tuple(x) for x in rec[:, :3].tolist()]


def _sweep_as_records(lines):
    return [(l[3], l[4], l[2]) for l in lines]


def _q6(ax, rec):
    return int(((rec[:, 3] - rec[:, 1] * 2 * (ax.rhoN + 2)) >= ax.rhoN + 2).sum())


@pytest.mark.parametrize("W,H,tl,th,rho,deg,thr", SIZES)
def test_numpy_emission_is_the_oracle_peak_scan(oracle, model, W, H, tl, th, rho, deg, thr):
    """The restated emission (SSE2 groups, scalar remainder with quirk Q6) gives the same multiset of records as orc_kht_peak_votes."""
    rc, e = oracle.canny(synth_frame(W, H, 99), tl, th)
    ax, counts, gs = model.vote_map(e, rho, deg)
    assert counts is not None
    rec = emission(ax, counts, thr)
    assert len(rec) > 0
    assert sorted(_records_as_lines(rec)) == sorted(map(tuple, model.oracle_votes(ax, counts, thr).tolist()))
    assert len(np.unique(rec[:, 3])) == len(rec) and rec[:, 3].max() < 2 ** 32          # emission keys are unique 32-bit values
    if ax.rhoN % 4 == 3:
        assert _q6(ax, rec) > 0


@pytest.mark.parametrize("W,H,tl,th,rho,deg,thr", SIZES)
def test_local_line_rule_is_the_sequential_sweep(oracle, model, W, H, tl, th, rho, deg, thr):
    """On the canonical (stably sorted) list, "no earlier record at another of the 8 positions around" picks exactly the lines of the reference's
    sweep, in the same order -- the locality the GPU peak kernel relies on."""
    rc, e = oracle.canny(synth_frame(W, H, 99), tl, th)
    ax, counts, gs = model.vote_map(e, rho, deg)
    rec = canonical(emission(ax, counts, thr))
    swept = _sweep_as_records(model.sweep(ax, rec[:, :3]))
    assert len(swept) > 0
    assert _records_as_lines(rec[local_lines(rec, ax.rhoN, ax.T)]) == swept
    ref, _ = oracle.kht(e, rho, deg, thr)
    assert sorted(l[2] for l in ref)[-1] == swept[0][2]                                   # the strongest line is the same in both orders


@pytest.mark.parametrize("rhoN", [2, 3, 4, 5, 7, 11, 15, 16, 19])
def test_local_line_rule_on_tie_heavy_count_maps(model, rhoN):
    """Synthetic vote maps full of ties -- including rhoN <= 4 (one scalar loop, no sign test) and rhoN % 4 == 3 (a Q6 record at position (theta, 1) next
    to, and at the same position as, main-scan records): emission multiset against the oracle, local rule against the sweep."""
    rng = np.random.RandomState(rhoN)
    T = 23
    ax = Axes(1.0, 0.0, 1.0, 0.0, rhoN, T, 0, 0)
    main_end, positive, q6 = scan(rhoN)
    for trial in range(6):
        counts = (rng.randint(0, 3, size=(T + 2, rhoN + 2)) * rng.randint(0, 2, size=(T + 2, rhoN + 2))).astype(np.int32)
        if trial % 2:
            counts[rng.rand(T + 2, rhoN + 2) < 0.1] *= -1                                 # sign test of the main scan vs the remainder's "!= 0"
        for thr in (1, 4, 9):
            rec = emission(ax, counts, thr)
            assert sorted(_records_as_lines(rec)) == sorted(map(tuple, model.oracle_votes(ax, counts, thr).tolist())), (trial, thr)
            rec = canonical(rec)
            assert _records_as_lines(rec[local_lines(rec, rhoN, T)]) == _sweep_as_records(model.sweep(ax, rec[:, :3])), (trial, thr)
    if q6 is not None:
        assert rhoN % 4 == 3


def test_the_new_symbols_are_exported():
    from compv_amd import capi
    lib = capi.load()
    for s in ("compvhip_plan_houghkht_ex", "compvhip_houghkht_ex_u8"):
        assert s in capi.EXPORTS and hasattr(lib, s), s


def test_null_plan_context_and_options_are_refused():
    from compv_amd import capi
    lib = capi.load()
    opts = capi.KhtOpts()
    opts.order = capi.KHT_ORDER_CANONICAL
    counts = np.zeros(1, np.uint64)
    lines = np.zeros(4, capi.LINE_DTYPE)
    assert lib.compvhip_plan_houghkht_ex(None, None, C.byref(opts), lines.ctypes.data_as(C.c_void_p), 4, counts.ctypes.data_as(C.c_void_p), None) \
        == capi.E_INVALID_PARAMETER
    assert lib.compvhip_plan_houghkht_ex(None, None, None, None, 0, None, None) == capi.E_INVALID_PARAMETER
    e = np.zeros((8, 8), np.uint8)
    n = C.c_size_t(0)
    assert lib.compvhip_houghkht_ex_u8(None, e.ctypes.data_as(C.c_void_p), 8, 8, 8, None, None, 0, C.byref(n), None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_houghkht_ex_u8(None, e.ctypes.data_as(C.c_void_p), 8, 8, 8, C.byref(opts), None, 0, C.byref(n), None) == capi.E_INVALID_PARAMETER


def test_python_order_keyword():
    from compv_amd import capi
    assert capi.KHT_ORDERS == {"reference": 0, "canonical": 1}
    assert C.sizeof(capi.KhtOpts) == 48                                                   # compvhip_kht_opts on LP64
    with pytest.raises(ValueError):
        capi._kht_order("stable")
