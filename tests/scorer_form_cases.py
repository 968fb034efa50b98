"""The case tables of the scorer kernels' dispatch forms (csrc/mgfn.hip: bn_rows, chan_layernorm, head_ln_fc, dwconv_t), with the
form each case must take when every operand is 16-byte aligned.  With an operand on a 4-byte boundary every launcher takes its
generic / scalar form (0).  tests/test_scorer_forms_host.py pins these expectations against the library's form queries without a
GPU; tests/test_hip_scorer_forms.py runs every case on the device against fp64."""

# advhip_bn_rows_form's answers (ADVHIP_BN_ROWS_* of include/advhip.h)
BN_GENERIC, BN_REG256X4, BN_REG256X12, BN_REG1024X4 = 0, 1, 2, 3
BN_FORM_NAMES = {BN_GENERIC: "generic", BN_REG256X4: "reg<256,4>", BN_REG256X12: "reg<256,12>", BN_REG1024X4: "reg<1024,4>"}

# (C, N, form when aligned)
BN_CASES = (
    [(c, n, BN_REG1024X4) for c in (3, 130) for n in (4, 4096, 4100, 16384)]
    + [(3, 16388, BN_GENERIC)]                                    # one quad past 1024 x 4 x 4
    + [(512, n, BN_REG256X4) for n in (4, 1024, 1028, 4096)]
    + [(512, n, BN_REG256X12) for n in (4100, 12288)]
    + [(512, 12292, BN_GENERIC)]                                  # one quad past 256 x 4 x 12
    + [(3, 6, BN_GENERIC), (512, 6, BN_GENERIC)]                  # N % 4 != 0
)
BN_BIG_MEAN = (130, 4100)  # the case whose input has its mean 40 standard deviations from zero

# (C, N, form when aligned): 0 = generic, else channels per thread of the 16-byte form
LN_CASES = (
    [(c, n, c // 64) for c in (64, 128, 1024) for n in (4, 28, 32, 36, 100)]
    + [(c, n, 0) for c in (3, 63, 65, 96) for n in (1, 5, 33)]
    + [(1024, 6, 0)]                                              # N % 4 != 0
)
LN_BIG_MEAN = (128, 36)

# (C, N, form when aligned): 0 = generic, 1 = the 16-byte form
HEAD_CASES = [(1024, 4, 1), (1024, 36, 1), (1024, 320, 1), (1024, 6, 0)]
HEAD_BIG_MEAN = (1024, 36)
HEAD_SATURATED = (1024, 36)  # the shape of the case with logits up to +-30

# (K, T, form when aligned): 0 = one element per thread, 1 = four consecutive t per thread
DW_CASES = [(k, t, 1) for k in (3, 5) for t in (4, 8, 12, 32)] + [(k, t, 0) for k in (3, 5) for t in (1, 2, 3, 5)]
DW_BIG_MEAN = (5, 12)
# (C, H, rows, advhip_dwconv_t_bwd_chunks(C, rows)): every (K, T) case runs on each
DW_GEOMETRIES = [(64, 4, 3, 1), (64, 4, 6, 2), (64, 4, 12, 4), (64, 4, 32, 32)]

COLSUM_ROWS = (1, 7, 8, 9, 56, 57, 64, 65, 121, 320)
COLSUM_COLS = (1, 31, 32, 33, 70)
COLSUM_PERIOD_COLS = (24, 72)  # multiples of both periods
COLSUM_PERIODS = (4, 6)

# every (query, form) the library can answer: what the GPU file's last test counts the cases against
ALL_FORMS = ([("bn_rows", f) for f in (BN_GENERIC, BN_REG256X4, BN_REG256X12, BN_REG1024X4)] + [("chan_layernorm", f) for f in (0, 1, 2, 16)]
             + [("head_ln_fc", f) for f in (0, 1)] + [("dwconv_t", f) for f in (0, 1)])


def query(lib, what, *args):
    """The library's answer: what = one of ALL_FORMS' names, args = (C, N, aligned16), for dwconv_t (T, aligned16)."""
    return int(getattr(lib, f"advhip_{what}_form")(*[int(a) for a in args]))
