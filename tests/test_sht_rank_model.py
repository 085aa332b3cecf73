"""The contract of the line sort (sht_sort_kernels.hip), on the CPU: ranks counted in order inside chunks, chunk histograms, the descending-strength scan and
the place arithmetic give numpy's stable sort on (-strength) -- for random and adversarial key sets, with and without the lineCap / maxLines cut.  The model
is tests/sht_rank_cases.py; the kernels are held against the oracle in tests/test_gpu_sht_rank.py."""
import numpy as np
import pytest

import sht_rank_cases as rc

KEY_SETS = rc.model_key_sets()


@pytest.mark.parametrize("name,strength,bits", KEY_SETS, ids=[k[0] for k in KEY_SETS])
def test_model_is_the_stable_sort_on_descending_strength(name, strength, bits):
    want = rc.stable_order(strength)
    got = rc.frame_order(strength, bits)
    assert got.tolist() == want.tolist(), name


@pytest.mark.parametrize("name,strength,bits", KEY_SETS, ids=[k[0] for k in KEY_SETS])
def test_model_cuts_are_prefixes_of_the_sorted_list(name, strength, bits):
    want = rc.stable_order(strength)
    n = len(strength)
    for cap, max_lines in ((max(1, n // 3), 0), (n + 5, max(1, n // 2)), (max(1, n - 1), max(1, n // 2 + 1)), (1, 1)):
        got = rc.frame_order(strength, bits, cap, max_lines)
        assert got.tolist() == want[:min(n, cap, max_lines if max_lines > 0 else n)].tolist(), (name, cap, max_lines)


def test_rank_is_the_count_of_earlier_equal_strengths():
    """the definition itself, quadratic, on a chunk with ties at every distance"""
    s = rc.tie_runs_at(3000, 8, [rc.ROW, rc.ROW * rc.WAVE_ROWS, 1024], 3) % 48
    rank, hist = rc.chunk_rank(s, 64)
    assert rank.tolist() == [int((s[:i] == s[i]).sum()) for i in range(s.size)]
    assert hist.tolist() == np.bincount(s, minlength=64).tolist()


def test_key_sets_are_what_their_names_say():
    sets = {k[0]: k[1] for k in KEY_SETS}
    assert len(set(sets["all equal, three chunks"].tolist())) == 1 and sets["all equal, three chunks"].size > 2 * rc.CHUNK
    assert len(set(sets["all distinct, one whole chunk"].tolist())) == rc.CHUNK
    t = sets["ties across rows, waves and chunks"]
    for edge in (rc.ROW, rc.ROW * rc.WAVE_ROWS, 1024, rc.CHUNK, 2 * rc.CHUNK):
        assert t[edge - 1] == t[edge] and (t == t[edge]).sum() >= 12, edge      # one run, on both sides of the boundary
    assert sets["exactly one chunk"].size == rc.CHUNK and sets["one chunk and a line"].size == rc.CHUNK + 1


def test_lattice_maps_are_isolated_points():
    W, H, step = rc.LATTICE
    m = rc.lattice_frame("three_chunks")
    assert int((m != 0).sum()) == (W // step) * (H // step)
    assert int((rc.lattice_frame("one_chunk") != 0).sum()) == rc.LATTICE_FRAMES["one_chunk"][0]
    assert not rc.lattice_frame("none").any()
