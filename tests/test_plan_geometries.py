"""CPU check of the plan geometry table (tests/plan_geometries.py): it must keep reaching every case the GPU sweep exists for."""
from plan_geometries import (CHUNK_SORT_MAX, FRAME_SLOT, GEOMETRIES, PLAN_WORD_COLS, RESOLVE_BAND_ROWS, RESOLVE_CHUNK_COLS, SWAR_COLS, SWAR_ROWS,
                             XCH_GEOMETRY, XCH_MARGIN, XCH_MIN_WAVES, coverage_mpw, has_coverage_gap, swar_waves, takes_exchange_path)


def _missing(what, ok):
    return [] if ok else [what]


def test_geometry_table_reaches_every_case(oracle):
    rows = GEOMETRIES
    for W, H, S, F, theta in rows + [XCH_GEOMETRY]:
        assert 3 <= W <= S and S % 8 == 0 and H >= 3 and F >= 1, (W, H, S, F)
    gap = [has_coverage_gap(W, oracle.canny_coverage(W)) for W, _, _, _, _ in rows]
    m = []
    m += _missing("a GAP width (W = 1 mod 16)", any(gap))
    m += _missing("a width without a gap", not all(gap))
    m += _missing("GAP rows are W = 1 (mod 16) or W <= 16", all((W % 16 == 1 or W <= 16) for (W, *_), g in zip(rows, gap) if g))
    for r in range(1, 8):
        m += _missing("W %% 8 == %d" % r, any(W % 8 == r for W, *_ in rows))
    m += _missing("W <= 16 (mpw = 8)", any(coverage_mpw(W) == 8 for W, *_ in rows))
    for edge, name in ((SWAR_COLS, "one SWAR tile"), (PLAN_WORD_COLS, "one plan word row"), (RESOLVE_CHUNK_COLS, "one resolve chunk")):
        m += _missing("W just past " + name, any(W % edge in (1, 2) and W > edge for W, *_ in rows))
    for edge, name in ((SWAR_ROWS, "a multiple of 24 (SWAR rows)"), (RESOLVE_BAND_ROWS, "a multiple of 64 (resolve band)")):
        m += _missing("H just past " + name, any(H % edge == 1 for _, H, *_ in rows))
    pads = [S - W for W, _, S, _, _ in rows]
    m += _missing("S - W == 1", 1 in pads)
    m += _missing("8 <= S - W <= 63", any(8 <= p <= 63 for p in pads))
    m += _missing("S - W >= 64", any(p >= 64 for p in pads))
    m += _missing("S % 16 == 0 (bytes_to_bits vector path)", any(S % 16 == 0 for _, _, S, _, _ in rows))
    m += _missing("S % 16 == 8 (bytes_to_bits byte path)", any(S % 16 == 8 for _, _, S, _, _ in rows))
    m += _missing("max(W, H) == 4095 (chunk sort limit)", any(max(W, H) == CHUNK_SORT_MAX for W, H, *_ in rows))
    m += _missing("max(W, H) == 4097 (library sort)", any(max(W, H) == CHUNK_SORT_MAX + 2 for W, H, *_ in rows))
    for F in (1, 2, 3, 9):
        m += _missing("F == %d" % F, any(f == F for *_, f, _ in rows))
    m += _missing("F > kFrameSlot", any(f > FRAME_SLOT for *_, f, _ in rows))
    for theta in (1.0, 0.5, 1.5, 2.0):
        m += _missing("theta %.1f" % theta, any(t == theta for *_, t in rows))
    m += _missing("a KHT row (F <= 9) with lines-sized frames", any(F <= 9 and W * H >= 100000 for W, H, _, F, _ in rows))
    assert not m, "the plan geometry table no longer reaches: " + "; ".join(m)


def test_exchange_path_geometry_is_over_its_threshold(oracle):
    W, H, S, F, _ = XCH_GEOMETRY
    assert swar_waves(W, H, F) >= XCH_MARGIN * XCH_MIN_WAVES
    assert takes_exchange_path(W, H, F) and not takes_exchange_path(W, H, F, ksize=5)
    assert not takes_exchange_path(W, H, 64)                                # the comparison plan of the GPU test
    assert has_coverage_gap(W, oracle.canny_coverage(W))
    assert W % SWAR_COLS == 1 and H % SWAR_ROWS == 1                        # last SWAR tile one column wide, last row tile one row tall
    assert S * H * F <= 160 << 20                                           # one input and one output buffer stay a modest share of HBM
    # the sweep's rows stay well below the threshold: the exchange path is this batch's alone
    assert not any(takes_exchange_path(W, H, F) for W, H, _, F, _ in GEOMETRIES)
