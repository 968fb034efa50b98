"""The case tables of the pooling kernels (csrc/pool.hip), each case with the kernel form it must reach: advhip_maxpool3d_form's
answer for the un-padded entry points, 0 (the generic kernel, the only one it has) for advhip_maxpool3d_padded_f32, and
advhip_global_avgpool_form's for the mean.  tests/test_pool_host.py pins these expectations against the library's queries without a
GPU and checks the reference on every case against torch; tests/test_hip_pool_edges.py runs every case on the device."""

GENERIC, ROW233, TEMPORAL = 0, 1, 2  # ADVHIP_MAXPOOL_* of include/advhip.h
FORM_NAMES = {GENERIC: "generic", ROW233: "row233", TEMPORAL: "temporal"}
AVG_STRIDED, AVG_BUTTERFLY = 0, 1    # advhip_global_avgpool_form's answers

K233, S222 = (2, 3, 3), (2, 2, 2)
K211, S211 = (2, 1, 1), (2, 1, 1)

# (name, (B, C, T, H, W), kernel, stride, form with a dense y)
MAXPOOL_CASES = [
    # the wave-per-row kernel: Wo = 1 and one live row in the workgroup of four
    ("233.w4", (1, 1, 2, 3, 4), K233, S222, ROW233),
    # 5 output rows: the second workgroup has one live wave; column 7, row 5 and frame 4 lie in no window
    ("233.rows5", (1, 1, 5, 6, 8), K233, S222, ROW233),
    # Wo = 62 and Wo = 63: every lane of the wave but the last two / the last one stores
    ("233.w126", (1, 3, 2, 5, 126), K233, S222, ROW233),
    ("233.w128", (2, 1, 3, 4, 128), K233, S222, ROW233),
    # 233.w4 has one output: the same geometry on 15 (sample, channel) pairs, so that it sees more than one window's worth of values
    ("233.w4.bc15", (3, 5, 2, 3, 4), K233, S222, ROW233),
    # just outside the rule: Wo = 64, and odd rows
    ("233.w130", (1, 2, 2, 5, 130), K233, S222, GENERIC),
    ("233.w127", (1, 2, 2, 5, 127), K233, S222, GENERIC),
    ("233.w129", (1, 2, 2, 5, 129), K233, S222, GENERIC),
    # the temporal kernel: an odd T (the last frame is unused), kt = 3 with overlapping windows, and 5 outputs in all -- three of the
    # four unrolled slots of every live thread are past the end
    ("t.k2", (3, 7, 5, 5, 11), K211, S211, TEMPORAL),
    ("t.k3", (1, 2, 7, 3, 5), (3, 1, 1), S211, TEMPORAL),
    ("t.five", (1, 1, 2, 1, 5), K211, S211, TEMPORAL),
    # generic oddities: a window flat in t, and the non-local block's (1,2,2)
    ("g.k123", (1, 3, 5, 7, 9), (1, 2, 3), (1, 1, 2), GENERIC),
    ("g.k122", (1, 3, 5, 7, 9), (1, 2, 2), (1, 2, 2), GENERIC),
]
MAXPOOL_CASE = {c[0]: c for c in MAXPOOL_CASES}

# (name, (B, C, T, H, W), kernel, stride, padding): advhip_maxpool3d_padded_f32, always the generic kernel
PADDED_CASES = (
    # the 8x8 stem pool on every H, W of {1, 2, 3, 7, 8}: windows that are mostly padding, odd and even extents
    [(f"p.133.{h}x{w}", (2, 3, 2, h, w), (1, 3, 3), (1, 2, 2), (0, 1, 1)) for h in (1, 2, 3, 7, 8) for w in (1, 2, 3, 7, 8)]
    # one frame under a 3-frame window, and padding of exactly half the window
    + [("p.333.T1", (1, 2, 1, 5, 6), (3, 3, 3), (2, 2, 2), (1, 1, 1)), ("p.222.half", (2, 2, 3, 4, 5), (2, 2, 2), (1, 1, 1), (1, 1, 1))]
)

# position sweeps: (name, (T, H, W), kernel, stride, padding, form) -- one sample per input position, one launch per geometry and value
SWEEPS = [
    ("sweep.233", (4, 5, 8), K233, S222, (0, 0, 0), ROW233),
    ("sweep.233.w128", (2, 3, 128), K233, S222, (0, 0, 0), ROW233),
    ("sweep.t", (4, 1, 6), K211, S211, (0, 0, 0), TEMPORAL),
    ("sweep.padded", (3, 4, 5), (2, 2, 2), (1, 1, 1), (1, 1, 1), GENERIC),
]

# y = channels [3, 3 + C) of C + 5 of a sentinel tensor, B = 2: (case, form with y padded).  A temporal shape must fall to the generic kernel.
YSLICE_CASES = [("233.w4", ROW233), ("233.rows5", ROW233), ("233.w126", ROW233), ("233.w128", ROW233), ("t.k2", GENERIC), ("g.k123", GENERIC)]
YSLICE_LO, YSLICE_WIDE, YSLICE_B = 3, 5, 2

# x one float into its allocation (a 4-byte boundary): the launcher does not look at alignment
OFF1_CASES = [("233.rows5", ROW233), ("233.w128", ROW233), ("t.k2", TEMPORAL)]

# the smallest totals past one sweep of each grid-stride loop: (name, shape, kernel, stride, form, outputs, outputs of one sweep)
GRID_CASES = [
    ("grid.generic", (1, 5, 1, 1030, 1640), (1, 2, 2), (1, 2, 2), GENERIC, 2_111_500, 8192 * 256),
    ("grid.temporal", (1, 65, 2, 256, 253), K211, S211, TEMPORAL, 4_209_920, 4096 * 256 * 4),
]

# advhip_global_avgpool_f32: every n x every number of rows (workgroups of four rows: 1, 3 and 5, 9 leave a partial last one)
MEAN_N = (1, 2, 63, 64, 65, 98, 127, 128, 129, 191, 192, 193, 4097)
MEAN_ROWS = (1, 3, 4, 5, 9)
MEAN_REAL_N = (98, 200)  # one real-valued case per form


def mean_form(n):
    return AVG_BUTTERFLY if n <= 128 else AVG_STRIDED


# the 8x8 head: x of shape (2, 65, T, H, W); in the first every axis equals its window
HEAD_GEOMETRIES = [(4, 7, 7), (5, 7, 7), (4, 8, 10), (8, 8, 10), (7, 13, 9)]
HEAD_HOST_GEOMETRIES = HEAD_GEOMETRIES + [(4, 14, 7)]
HEAD_TOO_SMALL = [(3, 7, 7), (4, 6, 7), (4, 7, 6)]
HEAD_BC = (2, 65)

ALL_FORMS = [("maxpool3d", f) for f in (GENERIC, ROW233, TEMPORAL)] + [("global_avgpool", f) for f in (AVG_STRIDED, AVG_BUTTERFLY)]


def maxpool_form(lib, shape, k, s, y_padded):
    """the library's answer for a launch of the un-padded entry points"""
    return int(lib.advhip_maxpool3d_form(int(shape[-1]), *[int(v) for v in k], *[int(v) for v in s], int(bool(y_padded))))


def avgpool_form(lib, n):
    return int(lib.advhip_global_avgpool_form(int(n)))
