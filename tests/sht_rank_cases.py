"""The line sort's contract as a numpy model, and the inputs the rank tests share (no GPU needed to import this).

sht_sort_kernels.hip orders a frame's lines -- strength descending, ties in emission order, i.e. a stable sort on (-strength) -- without sorting anything:

  rank     per chunk of CHUNK consecutive lines, for every line at its own position: the number of EARLIER lines of the chunk with the same strength.  A row of
           ROW lines is one wave: a line's rank inside the row is the number of lower lanes with its strength, the first lane of every group of equal strengths
           adds the group's size to count[strength] and what it reads back is the number of equal strengths in the earlier rows; rows in emission order.
  hist     count[] after the chunk's last row: lines per strength of the chunk
  scan     first slot of a strength in the frame: exclusive sum, in descending strength order, of the lines per strength over the frame's chunks
  place    slot = first slot of the strength + lines of that strength in the frame's earlier chunks + rank; written when slot < min(lines, lineCap, maxLines)

The model below does exactly these four steps; tests/test_sht_rank_model.py holds it against numpy's stable argsort, tests/test_gpu_sht_rank.py holds the
kernels against the CPU oracle on edge maps built for ties."""
import numpy as np

CHUNK = 8192          # kShtSortChunk
ROW = 64              # a wave
WAVE_ROWS = 8         # consecutive rows of a chunk that one wave of the rank kernel owns: a wave's lines end every 512
MAX_BITS = 13         # kShtSortMaxStrengthBits: strengths of max(W, H) <= 4095
KEY_CAP = 1 << 16     # key slots per frame of a plan whose caller asks for less (kMinLineCap)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------------
def chunk_rank(inv, bins):
    """(rank per line, histogram) of one chunk's inverted strengths in emission order, row by row as the kernel counts them"""
    inv = np.asarray(inv, np.int64)
    assert 0 < inv.size <= CHUNK
    count = np.zeros(bins, np.int64)
    rank = np.zeros(inv.size, np.int64)
    for r0 in range(0, inv.size, ROW):
        v = inv[r0:r0 + ROW]
        same = v[:, None] == v[None, :]                      # the ballots: lanes with my strength
        in_row = np.tril(same, -1).sum(1)                    # mbcnt: lower lanes of my group
        size = same.sum(1)
        first = same.argmax(1)                               # my group's first lane
        old = np.zeros(v.size, np.int64)
        for lane in np.flatnonzero(in_row == 0):             # one returning add per group
            old[lane] = count[v[lane]]
            count[v[lane]] += size[lane]
        rank[r0:r0 + ROW] = old[first] + in_row
    return rank, count


def frame_order(strength, bits, line_cap=None, max_lines=0):
    """The model's sorted list of one frame: indices into `strength` (emission order), slot by slot, for the min(lines, lineCap, maxLines) slots that are written"""
    strength = np.asarray(strength, np.int64)
    n = strength.size
    limit = n if line_cap is None else min(n, line_cap)
    if max_lines > 0:
        limit = min(limit, max_lines)
    if n == 0:
        return np.zeros(0, np.int64)
    bins = 1 << bits
    assert strength.min() >= 0 and strength.max() < bins
    inv = (bins - 1) - strength
    chunks = -(-n // CHUNK)
    rank = np.zeros(n, np.int64)
    hist = np.zeros((chunks, bins), np.int64)
    for c in range(chunks):
        rank[c * CHUNK:(c + 1) * CHUNK], hist[c] = chunk_rank(inv[c * CHUNK:(c + 1) * CHUNK], bins)
    assert hist.max() < 65536                                # the chunk histogram is u16
    total = hist.sum(0)
    start = np.cumsum(total) - total                         # exclusive, ascending inverted strength = descending strength
    earlier = np.cumsum(hist, 0) - hist                      # [c][inv]: lines of that strength in the frame's earlier chunks
    i = np.arange(n)
    pos = start[inv] + earlier[i // CHUNK, inv] + rank
    assert sorted(pos.tolist()) == list(range(n)), "the slots are not a permutation"
    out = np.full(limit, -1, np.int64)
    keep = pos < limit
    out[pos[keep]] = i[keep]
    return out


def stable_order(strength):
    return np.argsort(-np.asarray(strength, np.int64), kind="stable")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# key sets for the model
# ---------------------------------------------------------------------------------------------------------------------------------------------
def tie_runs_at(n, bits, edges, seed):
    """random strengths with a run of one strength (unused elsewhere) laid across every index in `edges`"""
    rng = np.random.default_rng(seed)
    s = rng.integers(1, (1 << bits) - 64, n)
    for k, e in enumerate(edges):
        if e < n:
            s[max(0, e - 5 - k):min(n, e + 7 + k)] = (1 << bits) - 1 - k
    return s


def model_key_sets():
    """[(name, strengths in emission order, strength bits)]"""
    rng = np.random.default_rng(7)
    big = 2 * CHUNK + 777
    sets = [
        ("one line", np.array([5]), 4),
        ("all equal, three chunks", np.full(big, 3), MAX_BITS),
        ("all distinct, one whole chunk", rng.permutation(CHUNK), MAX_BITS),
        ("all distinct, ascending", np.arange(1, 5000), MAX_BITS),
        ("two strengths alternating", np.where(np.arange(big) % 2 == 0, 2, 9), 4),
        ("two strengths alternating by rows", np.where((np.arange(big) // ROW) % 2 == 0, 2, 3), 2),
        ("random, few strengths", rng.integers(1, 8, big), 3),
        ("random, every strength", rng.integers(0, 1 << MAX_BITS, big), MAX_BITS),
        ("random, 12 bits", rng.integers(0, 1 << 12, CHUNK + 1), 12),
        ("ties across rows, waves and chunks", tie_runs_at(big, MAX_BITS, [ROW, ROW * WAVE_ROWS, 1024, CHUNK, 2 * CHUNK], 11), MAX_BITS),
        ("exactly one chunk", rng.integers(1, 40, CHUNK), 6),
        ("one chunk and a line", rng.integers(1, 40, CHUNK + 1), 6),
        ("one row short of a chunk", rng.integers(1, 40, CHUNK - ROW + 1), 6),
    ]
    return sets


# ---------------------------------------------------------------------------------------------------------------------------------------------
# edge maps for the kernels: isolated points on a lattice; at threshold 1 thousands of accumulator cells are lines of strength 2, 3, 4 ...
# ---------------------------------------------------------------------------------------------------------------------------------------------
def lattice_map(W, H, step, keep=None, seed=0):
    """(H, W) uint8 edge map: the `keep` points of a lattice of pitch `step` with the smallest hash (integer arithmetic only: the same map everywhere)"""
    ys, xs = np.mgrid[step // 2:H:step, step // 2:W:step]
    ys, xs = ys.ravel(), xs.ravel()
    h = (np.arange(ys.size, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    order = np.argsort(h, kind="stable")[:ys.size if keep is None else keep]
    m = np.zeros((H, W), np.uint8)
    m[ys[order], xs[order]] = 255
    return m


LATTICE = (512, 512, 16)                                      # W, H, pitch: 1024 points
# name -> (keep, seed, lines at threshold 1 under the oracle); found by search on the CPU, asserted by the GPU test before it runs anything
LATTICE_FRAMES = {
    "one_chunk": (296, 93, CHUNK),
    "one_chunk_and_a_line": (298, 62, CHUNK + 1),
    "three_chunks": (None, 0, 23669),                        # 2 * CHUNK + 7285
    "none": (0, 0, 0),
}


def lattice_frame(name):
    W, H, step = LATTICE
    keep, seed, _ = LATTICE_FRAMES[name]
    return lattice_map(W, H, step, keep, seed)


def emission_order(lines):
    """oracle lines (rho, theta, strength, row, col) in nms_apply's order: accumulator row, then column"""
    return sorted(lines, key=lambda l: (l[3], l[4]))


def tie_distances(strengths):
    """of a frame's strengths in emission order: does some strength occur twice in one row, in adjacent rows, and in rows far apart (>= 64 rows) of one chunk?"""
    s = np.asarray(strengths[:CHUNK])
    rows = np.arange(s.size) // ROW
    found = {"row": False, "adjacent": False, "far": False}
    for v in np.unique(s):
        r = rows[s == v]
        d = np.diff(r)
        found["row"] |= bool((d == 0).any())
        found["adjacent"] |= bool((d == 1).any())
        found["far"] |= bool(r.size > 1 and r[-1] - r[0] >= 64)
    return found
