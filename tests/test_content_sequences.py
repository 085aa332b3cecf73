"""The sequences of tests/content_sequences.py have the properties tests/test_gpu_content_sequences.py relies on -- checked here on the CPU with the oracle and
the stage models, so that a sequence which lost one (a retuned threshold, another seed) is found as a bug of the test, without a GPU."""
import numpy as np
import pytest

import content_sequences as cs
import plan_geometries as geo


def canny_of(oracle, img, prm):
    if prm["mode"] == cs.OTSU:
        lo, hi = oracle.otsu_canny_thresholds(oracle.otsu(img), prm["tl"], prm["th"])
        rc, e = oracle.canny(img, float(lo), float(hi), prm["ksize"])
    else:
        rc, e = oracle.canny(img, prm["tl"], prm["th"], prm["ksize"], prm["mode"])
    assert rc == 0
    return e


def test_every_step_rotates_the_classes():
    for classes in (3, 4, 5):
        for k in range(2 * classes):
            kinds = [cs.class_of(k, f, classes) for f in range(cs.F)]
            assert len(set(kinds)) == cs.F                                   # three different classes in a batch
            assert [cs.class_of(k + 1, f, classes) for f in range(cs.F - 1)] == kinds[1:]   # a frame takes over its neighbour's class
    assert cs.run_order([0, 1, 2]) == [0, 1, 2, 0]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_geometries_are_ragged_padded_and_cover_both_gap_kinds(oracle):
    gaps = set()
    for W, H, S in cs.PLAN_GEOMETRIES:
        assert W % 8 != 0 and S > W and S % 8 == 0
        assert -(-W // 496) >= 2                                             # at least two 496-column Canny tiles per row
        assert H > geo.SWAR_ROWS                                             # more than one SWAR row tile
        gaps.add(geo.has_coverage_gap(W, oracle.canny_coverage(W)))
    assert gaps == {False, True}
    # one geometry has several resolve bands AND several resolve chunks per frame: the hysteresis workgroups read their neighbours' change flags
    assert any(H > geo.RESOLVE_BAND_ROWS and W > geo.RESOLVE_CHUNK_COLS for W, H, S in cs.PLAN_GEOMETRIES)


def test_plan_parameters_change_between_steps():
    P = cs.PLAN_PARAMS
    for a, b in zip(P, P[1:] + P[:1]):
        assert (a["ksize"], a["mode"], a["tl"], a["th"]) != (b["ksize"], b["mode"], b["tl"], b["th"]) and a["thr"] != b["thr"]
    assert {p["ksize"] for p in P} == {3, 5} and {p["mode"] for p in P} == {cs.GRADIENT, cs.PERCENT_OF_MEAN, cs.OTSU}
    assert any(p["max_lines"] > 0 for p in P) and any(p["max_lines"] == 0 for p in P)
    assert all(a["ksize"] != b["ksize"] for a, b in zip(P, P[1:]))           # ksize 3 <-> 5 at every step


@pytest.mark.parametrize("W,H,S", cs.PLAN_GEOMETRIES, ids=lambda v: str(v))
def test_plan_sequence_classes_do_what_they_are_there_for(oracle, W, H, S):
    from compv_amd import capi
    nx, ny, _ = capi.houghsht_vote_grid(W, H, 1.0, cs.F)                     # host arithmetic: no GPU
    TW, TH = cs.vote_tile_size(W, H, nx, ny)
    steps = cs.plan_sequence(W, H)
    seen = {}
    accs = {}
    for k, (frames, prm) in enumerate(steps):
        assert len(set(prm["kinds"])) == cs.F
        for f, kind in enumerate(prm["kinds"]):
            e = canny_of(oracle, frames[f], prm)
            acc = oracle.sht_acc(e, 1.0)
            lines = oracle.sht_lines_from_acc(acc, W, H, 1.0, prm["thr"])
            accs[(k, f)] = (acc, lines)
            assert len(lines) <= 65536                                       # the key buffer's contract (compv_hip.h): beyond it the line set is arbitrary
            seen.setdefault(kind, []).append(len(lines))
            if kind == "constant":
                assert not e.any() and not acc.any() and not lines           # no edges, no lines
            elif kind == "noise":
                assert (e != 0).mean() > 0.2 and len(lines) > 100            # dense
            else:
                # some (tile, theta) column of the vote holds a count of 256 or more: the tile's own share of the votes is the accumulator of its pixels alone
                share = 0
                for ty in range(ny):
                    for tx in range(nx):
                        m = np.zeros_like(e)
                        m[ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW] = e[ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW]
                        share = max(share, int(oracle.sht_acc(m, 1.0).max()))
                assert share >= 256, (k, f, kind, share)
                assert len(lines) > 0
    assert set(seen) == set(cs.PLAN_CLASSES)
    # the shifted bars: cells that were peaks (lines) of the same frame's bars two steps earlier are exactly zero now, next to cells that are not
    checked = 0
    for (k, f), (acc, lines) in accs.items():
        if steps[k][1]["kinds"][f] != "shifted" or (k - 2, f) not in accs:
            continue
        assert steps[k - 2][1]["kinds"][f] == "bars" and steps[k - 1][1]["kinds"][f] == "constant"
        gone = [(l[3], l[4]) for l in accs[(k - 2, f)][1] if acc[l[3], l[4]] == 0]
        assert gone, (k, f)
        assert any(acc[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2].any() for r, c in gone), (k, f)   # the 3 x 3 window of the NMS
        checked += 1
    assert checked >= 2
    # ... and every frame meets the constant frame right after a bars class (the stale high bytes would show there first)
    for f in range(cs.F):
        kinds = [p["kinds"][f] for _, p in steps]
        assert any(a == "bars" and b == "constant" for a, b in zip(kinds, kinds[1:] + kinds[:1])), (f, kinds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (b)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_sort_sequence_line_counts_sit_either_side_of_the_chunks(oracle):
    W, H, S = cs.SORT_GEOMETRY
    R, T, _ = oracle.sht_dims(W, H, 1.0)
    assert R * T > cs.SORT_CHUNK * cs.SORT_MAX_CHUNKS                        # a line capacity can pass 32 chunks (it is clamped to R * T)
    assert cs.SORT_BIG_CAP > cs.SORT_CHUNK * cs.SORT_MAX_CHUNKS == 131072 and cs.SORT_BIG_CAP <= R * T
    assert max(W, H) <= geo.CHUNK_SORT_MAX and W % 8 != 0 and S > W          # a plan that starts on the device sort
    steps = cs.sort_sequence()
    assert [p["line_cap"] for _, p in steps][:3] == [16, 10000, 16]
    want = {"three_chunks": lambda n: n > 2 * cs.SORT_CHUNK and n % cs.SORT_CHUNK, "part_chunk": lambda n: 0 < n < cs.SORT_CHUNK, "none": lambda n: n == 0,
            "two_chunks": lambda n: cs.SORT_CHUNK < n < 2 * cs.SORT_CHUNK}
    for f in range(cs.F):
        kinds = [p["kinds"][f] for _, p in steps]
        assert kinds[:4] == [cs.SORT_CLASSES[(k + f) % 4] for k in range(4)]
    for k, (maps, prm) in enumerate(steps):
        for f, kind in enumerate(prm["kinds"]):
            n = len(oracle.sht(maps[f], 1.0, 1))
            assert want[kind](n), (k, f, kind, n)
            assert n <= 65536
    # frame 0 goes > 2 x 4096, < 4096, none, > 4096: the chunks that return at once hold the histograms of the call before
    assert [p["kinds"][0] for _, p in steps] == ["three_chunks", "part_chunk", "none", "two_chunks"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (e)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["own_train", "shared_train"])
def test_match_sequence_slice_counts_and_good_lists(shared):
    import match_model as mm
    m = cs.MATCH
    assert cs.match_slices(m["tcap"]) >= 3 and cs.match_slices(m["qcap"]) >= 3     # the handle spans three forward AND three reverse slices
    steps = cs.match_steps(shared)
    assert [s["kind"] for s in steps][:5] == ["all_slices", "one_slice", "no_train", "no_query", "all_slices"]
    assert [s["cross_check"] for s in steps] == [True, True, False, True, False, True]
    query, train = cs.match_descriptors(shared)
    assert query.shape == (m["pairs"], m["qcap"], m["q_stride"]) and m["q_stride"] > m["desc_bytes"] < m["t_stride"]
    B = m["desc_bytes"]
    removed = 0
    for k, s in enumerate(steps):
        slices = [cs.match_slices(t) for t in s["t"]]
        want = {"all_slices": 3, "one_slice": 1, "no_train": 0}.get(s["kind"])
        if want is not None:
            assert slices == [want] * len(slices), (k, slices)
        if s["kind"] == "no_query":
            assert not any(s["q"]) and all(s["t"])
        elif s["kind"] != "no_train":
            assert len(set(s["q"])) == len(s["q"]) and all(s["q"])          # ragged: a count of its own for every pair
            if not shared:
                assert len(set(s["t"])) == len(s["t"])
        for p in range(m["pairs"]):
            q, t = query[p, :s["q"][p], :B], train[0 if shared else p, :s["t"][0 if shared else p], :B]
            plain = mm.good(q, t, m["knn"])
            assert len(plain) == (len(q) if len(t) else 0)
            if s["cross_check"] and len(q) > 1 and len(t):
                removed += len(plain) - len(mm.good(q, t, m["knn"], cross_check=True))
    assert removed > 0                                                       # the cross check decides something
    # the reverse pass (roles swapped) runs ceil(Q / 128) slices: under the cross check 3 everywhere, then 1 everywhere over a smaller non-zero train side, then
    # none, then 1, 2 and 3 side by side -- with steps in between that leave the reverse lists alone
    reverse = [[cs.match_slices(q) for q in s["q"]] for s in steps if s["cross_check"]]
    assert reverse[0] == [3, 3, 3] and reverse[1] == [1, 1, 1] and reverse[2] == [0, 0, 0] and sorted(reverse[3]) == [1, 2, 3], reverse
    assert 0 < max(steps[1]["t"]) <= cs.MATCH_SLICE < min(steps[0]["t"])       # a train side that has shrunk, not vanished, under the cross check
    if not shared:                                                           # the counts rotate: every pair takes the largest train count of the all-slices steps once
        assert steps[0]["t"] != steps[4]["t"] and sorted(steps[0]["t"]) == sorted(steps[4]["t"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (f)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_homography_sequence_has_status_1_and_status_2_steps():
    import homography_model as hm
    steps = cs.homography_sequence()
    assert [p["tries"] for _, p in steps] == [257, 63, 257, 63, 257]
    assert [p["given_quads"] for _, p in steps][:3] == [False, True, False]
    assert {p["mask"] for _, p in steps} == {True, False}
    want = {"planted_large": 0, "planted_other": 0, "four_points": 0, "three_points": 2, "collinear": 1}
    for pair in range(cs.HOMOGRAPHY["pairs"]):
        kinds = [p["kinds"][pair] for _, p in steps]
        assert any(a.startswith("planted") and b in ("three_points", "collinear") for a, b in zip(kinds, kinds[1:] + kinds[:1])), kinds
    for k, (sets, prm) in enumerate(steps):
        for pair, (s, d) in enumerate(sets):
            assert len(s) <= cs.HOMOGRAPHY["point_cap"] and prm["tries"] <= cs.HOMOGRAPHY["max_tries"]
            e = hm.find(s, d, len(s), prm["tries"], seed=prm["seed"], pair=pair)
            kind = prm["kinds"][pair]
            assert e["result"]["status"] == want[kind], (k, pair, kind)
            if kind == "collinear":                                          # every quad collinear: no try scores anything
                assert not np.asarray(e["counts"]).any() and e["result"]["bestTry"] == -1
            if kind == "planted_large":
                assert len(s) == 129 and e["result"]["inliers"] > 64
            if kind == "four_points":
                assert len(s) == 4 and e["result"]["inliers"] == 4
            if kind == "three_points":
                assert len(s) == 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (d)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", cs.FAST_GEOMETRIES, ids=lambda g: str(g))
def test_fast_sequence_counts_and_a_cut_at_a_tie(geom):
    import fast_model as fm
    W, H, S, F = geom
    assert (W, H) == (40, 37) or (W % 8 and S > W)
    steps = cs.fast_sequence(W, H)
    P = [p for _, p in steps]
    assert {p["N"] for p in P} == {9, 12} and {p["nonmax"] for p in P} == {True, False} and len({p["t"] for p in P}) >= 3
    assert all(a["scores"] != b["scores"] for a, b in zip(P, P[1:]))         # the caller's score map, then the plan's, ...
    assert {p["records"] for p in P} == {True, False}
    tie_cut = False
    where = {}
    for k, (fr, p) in enumerate(steps):
        for f, kind in enumerate(p["kinds"]):
            rec = fm.fast(fr[f], p["t"], p["N"], p["nonmax"])[0]
            if kind == "none":
                assert len(rec) == 0
            if kind == "many":
                assert len(rec) > 40
            if kind == "handful":
                assert 0 < len(rec) <= 4
                where.setdefault(f, []).append(sorted((int(r["x"]), int(r["y"])) for r in rec))
            if p["max_features"] > 1 and len(rec) > p["max_features"]:
                cut = fm.cut(rec, p["max_features"])
                tie_cut |= len(cut) > p["max_features"]                      # the cut falls inside a run of equal strengths: the whole run stays
    assert tie_cut
    assert all(a != b for w in where.values() for a, b in zip(w, w[1:]))     # the handful sits at other positions every time


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (g)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_scratch_sequences_change_what_the_scratch_holds(oracle):
    import hog_model as hm
    W, H, S = cs.SCRATCH_GEOMETRY
    assert W % 8 and S > W and W > 256 and H > 64
    levels = [[int(oracle.otsu(f)) for f in fr] for fr, _ in cs.otsu_sequence()]
    for f in range(cs.F):
        col = [lv[f] for lv in levels]
        assert all(abs(a - b) >= 15 for a, b in zip(col, col[1:])), col       # quite different histograms from call to call
    hists = [oracle.hist256(f) for f in cs.otsu_sequence()[0][0]]
    assert any((h != 0).sum() == 1 for h in hists)                           # the constant frame: one bin
    M = cs.MORPH_STEPS
    assert {p["call"] for p in M} == {"morph", "adaptive"} and {p["op"] for p in M if p["call"] == "morph"} == {cs.OPEN, cs.CLOSE}
    assert len({p["strel"] for p in M if p["call"] == "morph"}) == 4 and {p["border"] for p in M if p["call"] == "morph"} == {cs.BORDER_ZERO, cs.BORDER_REPLICATE}
    assert len({p["block"] for p in M if p["call"] == "adaptive"}) == 2
    geo = [hm.geometry(*cs.HOG_SIZE, hm.resolve(p["opts"])) for _, p in cs.hog_sequence()]
    assert all(g is not None for g in geo)
    maps = [g["cellsX"] * g["cellsY"] * p["nbins"] for g, p in zip(geo, cs.HOG_STEPS)]
    assert all(a != b for a, b in zip(maps, maps[1:]))                       # another cell-map layout at every call
    assert len({p["nbins"] for p in cs.HOG_STEPS}) >= 4 and len({p["cellW"] for p in cs.HOG_STEPS}) >= 4 and len({p["blockNorm"] for p in cs.HOG_STEPS}) == 5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (c)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_feature_parameters_change_and_a_dense_frame_precedes_an_empty_one(oracle):
    P = cs.FEATURE_PARAMS
    assert len(P) == len(cs.PLAN_PARAMS)
    assert [p["conn"] for p in P] == [8, 4, 8, 4, 8]                         # connectivity alternates
    for key in ("min_length", "max_gap", "half_width", "min_pixels"):
        assert all(a[key] != b[key] for a, b in zip(P, P[1:])), key
    assert [cap for _, cap in cs.FEATURE_OUTPUTS][:2] == [0, 64] and [lab for lab, _ in cs.FEATURE_OUTPUTS] == [False, True, False]
    W, H, S = cs.PLAN_GEOMETRIES[0]
    steps = cs.plan_sequence(W, H)
    for f in range(cs.F):
        kinds = [p["kinds"][f] for _, p in steps]
        k = next(i for i, (a, b) in enumerate(zip(kinds, kinds[1:])) if b == "constant")
        dense = canny_of(oracle, steps[k][0][f], steps[k][1])
        assert (dense != 0).sum() > 10000                                    # large stale numbers in segPerLine / compRows when the empty frame comes


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (h)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_kht_sequence_is_busy_empty_busy_with_other_lines(oracle):
    from kht_canon_model import CanonModel
    model = CanonModel(oracle)
    steps = cs.kht_sequence()
    assert [p["order"] for _, p in steps] == ["reference", "canonical", "reference", "canonical"]
    groups = [p["group"] for _, p in steps]
    assert any(g is not None and -(-cs.F // g) > 1 for g in groups) and None in groups     # a step whose batch is split into several groups
    seen = {}
    for k, (maps, p) in enumerate(steps):
        for f, kind in enumerate(p["kinds"]):
            ref, gs = oracle.kht(maps[f], 1.0, 1.0, p["threshold"])
            canon = model.lines(maps[f], threshold=p["threshold"])[0]
            if kind == "empty":
                assert not maps[f].any() and len(ref) == 0 and len(canon) == 0
            else:
                assert len(ref) >= 5 and len(canon) >= 5, (k, f, kind)
                seen.setdefault(f, []).append({(l[3], l[4]) for l in ref})
    for f, sets in seen.items():
        assert all(a != b for a, b in zip(sets, sets[1:])), f               # other lines every time a frame slot is busy
    for f in range(cs.F):
        kinds = [p["kinds"][f] for _, p in steps]
        assert any(a == "busy" and b == "empty" for a, b in zip(kinds, kinds[1:] + kinds[:1]))


def test_orb_sequences_go_many_none_handful():
    import orb_model as om
    import orb_pyramid_model as pm
    for W, H, S, F in cs.ORB_GEOMETRIES:
        steps = cs.orb_sequence(W, H)
        P = [p for _, p in steps]
        assert all(a["blur"] != b["blur"] or not (a["records"] and b["records"]) for a, b in zip(P, P[1:]))
        assert {p["blur"] for p in P if p["records"]} == {True, False} and {p["records"] for p in P} == {True, False} and {p["level"] for p in P} == {0, 1}
        for f in range(F):
            assert {p["counts"][f] for p in P} == set(cs.ORB_COUNTS) and {p["kinds"][f] for p in P} == set(cs.ORB_CLASSES)
        assert om.admissible(W // 2, H // 2, W, H)
    W, H, S, levels, sf, mf = cs.ORBPYR_GEOMETRY
    geo = pm.geometry(W, H, levels, sf, mf)
    assert levels >= 4 and not any(g["empty"] for g in geo) and S > W
    where = {}
    cut = False
    sizes = {"many": [], "handful": []}
    for k, (fr, p) in enumerate(cs.orbpyr_sequence()):
        for f, kind in enumerate(p["kinds"]):
            keys, lc, lk, planes = pm.detect(fr[f], levels, sf, 20, 9, True, mf, None)
            if kind == "none":
                assert len(keys) == 0 and not lk.any()
            elif kind == "many":
                assert (lk > 0).all() and (lc > 0).sum() >= 3               # corners on every level, survivors on three at least
                cut |= bool((lk > lc).any())
                sizes["many"].append(len(keys))
            else:
                assert 0 < len(keys) <= 5 * levels and (lc > 0).sum() >= 4
                where.setdefault(f, []).append(sorted((float(x), float(y)) for x, y in zip(keys["x"], keys["y"])))
                sizes["handful"].append(len(keys))
    assert cut
    assert min(sizes["many"]) > 4 * max(sizes["handful"]), sizes            # the lists really shrink: many -> none -> a handful
    assert all(a != b for w in where.values() for a, b in zip(w, w[1:]))
