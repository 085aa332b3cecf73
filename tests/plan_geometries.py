"""Geometries of the batched-plan sweep (tests/test_gpu_plan_geometry.py) and the launcher arithmetic that decides which kernel
instances they reach.  Importable without a GPU: tests/test_plan_geometries.py checks on the CPU that the table still reaches every
case listed below, so that trimming it later says what was dropped.

A row is (W, H, S, F, theta_deg): W x H frames at row stride S (S % 8 == 0, S > W), F frames, SHT theta step in degrees.
"""
import math

# canny_swar_kernels.hip: kSwCols output columns and SWAR_ROWS rows per wave tile; one wave per workgroup
SWAR_COLS = 240
SWAR_ROWS = 24
# launch_swar (canny_swar_kernels.hip:522): the 3x3 kernel takes the LDS exchange load path (XCH) when the launch has at least
# four times the chip's 8192 wave slots
XCH_MIN_WAVES = 4 * 8192
PLAN_WORD_COLS = 512       # compvhip_plan_create: 512 columns (16 mask words) per plan tile of the bit masks
RESOLVE_CHUNK_COLS = 2048  # canny_resolve_kernel: columns per workgroup chunk (kBandWords mask words)
RESOLVE_BAND_ROWS = 64     # canny_resolve_kernel: rows per band (kBandH)
CHUNK_SORT_MAX = 4095      # the device chunk sort of the line keys serves max(W, H) <= 4095; beyond, the library sort
FRAME_SLOT = 32            # kFrameSlot (kernels.hpp): per-frame counter slots


def swar_waves(W, H, F):
    """Waves of one SWAR Canny tile launch over F frames (launch_swar with kWaves = 1)."""
    return F * math.ceil(H / SWAR_ROWS) * math.ceil(W / SWAR_COLS)


def takes_exchange_path(W, H, F, ksize=3):
    return ksize == 3 and swar_waves(W, H, F) >= XCH_MIN_WAVES


def has_coverage_gap(W, coverage):
    """enqueueCanny's GAP flag from the reference's column coverage (simdEnd, cStart) = cannyCoverage(W): the SIMD piece
    [1, simdEnd) and the scalar remainder [cStart, W - 1) leave a hole between them."""
    simd_end, c_start = coverage
    return not (simd_end >= W - 1 or c_start <= simd_end)


def coverage_mpw(W):
    """Columns per SIMD step of the reference's coverage: 16, or 8 when W - 1 < 16, or 1 below 9 columns."""
    return 16 if W - 1 >= 16 else (8 if W - 1 >= 8 else 1)


GEOMETRIES = [
    (9, 9, 16, 3, 1.0),          # W = 9: mpw = 8 and the coverage is empty (GAP); the smallest frame; S - W = 7, S % 16 == 0
    (17, 9, 24, 2, 0.5),         # W = 17 = 1 (mod 16): the first GAP width with mpw = 16; S % 16 == 8 (bytes_to_bits' byte path)
    (13, 70, 24, 2, 1.5),        # W % 8 == 5, W <= 16 without a gap (mpw = 8); H just past one resolve band (64); S - W = 11
    (50, 27, 64, 1, 2.0),        # W % 8 == 2; a single frame; H just past one SWAR row tile (24); S - W = 14
    (43, 49, 48, 2, 2.0),        # W % 8 == 3; H just past two SWAR row tiles; S - W = 5
    (239, 24, 240, 5, 1.0),      # W % 8 == 7, one column short of a SWAR tile, exactly one row tile; S - W = 1
    (241, 25, 248, 3, 1.5),      # GAP; one column past a SWAR tile (the second tile is one column wide); H = 24 + 1; S % 16 == 8
    (166, 89, 176, 3, 0.5),      # W % 8 == 6; H past 64 and past 3 x 24; S - W = 10, S % 16 == 0
    (513, 65, 576, 9, 1.0),      # GAP; one column past a plan word row (512); H past a resolve band; F = 9 (a second XCD group); S - W = 63
    (641, 480, 720, 4, 0.5),     # GAP; S - W = 79 >= 64
    (1001, 333, 1008, 33, 1.0),  # F = 33 > kFrameSlot (32); W % 8 == 1 without a gap; S - W = 7
    (2049, 130, 2112, 2, 2.0),   # GAP; one column past a resolve chunk (2048); H past 2 x 64; S - W = 63
    (4095, 70, 4096, 2, 1.0),    # max(W, H) = 4095: the largest frame on the chunk sort; W % 8 == 7; S - W = 1
    (4097, 33, 4104, 2, 1.5),    # max(W, H) = 4097: the library sort; GAP; S % 16 == 8
    (100, 1537, 104, 3, 1.0),    # tall frame: H = 1537 is just past 64 x 24 (both a SWAR row tile and a resolve band); W % 8 == 4
]

# The exchange-path batch: GAP with ragged W and H -- three SWAR tiles, the last one column wide, and five row tiles, the last one
# row tall -- and enough frames to put the launch 20 % over XCH_MIN_WAVES (about 128 MB of frames).
XCH_GEOMETRY = (481, 97, 488, 2731, 1.0)
XCH_MARGIN = 1.2
