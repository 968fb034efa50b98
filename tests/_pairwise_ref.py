"""numpy's float32 `np.linalg.norm(x, axis=-1)` restated operation by operation, vectorised over rows: the arithmetic
`advhip_add_magnitude_np_f32` reproduces bit for bit (include/advhip.h states the rule).

    s[i] = x[i] * x[i]                      rounded to fp32 on its own
    sum  = 0.0f + pw(s, C)                  numpy's pairwise sum: blocks of at most 128, eight accumulators each
    out  = sqrt(sum)                        correctly rounded

Valid for C <= 8192 (numpy reduces in chunks of 8192 elements; the order changes above that).
"""
import numpy as np

PW_BLOCK = 128
MAX_C = 8192


def split(n: int) -> int:
    """Length of the left half of a block of n > 128 elements."""
    n2 = n // 2
    return n2 - n2 % 8


def pairwise_sum(a: np.ndarray) -> np.ndarray:
    """(rows, n) float32 -> (rows,) float32: numpy's pairwise_sum of every row, every add rounded to fp32."""
    assert a.dtype == np.float32 and a.ndim == 2
    n = a.shape[1]
    if n < 8:
        res = np.zeros(a.shape[0], np.float32)
        for i in range(n):
            res = res + a[:, i]
        return res
    if n <= PW_BLOCK:
        r = [a[:, j].copy() for j in range(8)]
        whole = n - n % 8
        for i in range(8, whole, 8):
            for j in range(8):
                r[j] = r[j] + a[:, i + j]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(whole, n):
            res = res + a[:, i]
        return res
    n2 = split(n)
    return pairwise_sum(a[:, :n2]) + pairwise_sum(a[:, n2:])


def norm_rows(x: np.ndarray) -> np.ndarray:
    """(..., C) float32 -> (...) float32, the bits of np.linalg.norm(x, axis=-1)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.shape[-1] <= MAX_C
    flat = x.reshape(-1, x.shape[-1])
    with np.errstate(all="ignore"):
        s = flat * flat
        total = np.float32(0.0) + pairwise_sum(s)
        return np.sqrt(total).astype(np.float32).reshape(x.shape[:-1])


def add_magnitude(x: np.ndarray, transpose: bool = False) -> np.ndarray:
    """(a, b, C) -> (a, b, C+1), or (b, a, C+1) with `transpose`: what the kernel writes."""
    out = np.concatenate((x, norm_rows(x)[..., None]), axis=2)
    return np.ascontiguousarray(out.transpose(1, 0, 2)) if transpose else out


def leaves(C: int):
    """[(start, len, adds)] in order: the blocks of at most 128 elements the recursion ends in, and after how many of them a
    pending partial sum is added (the post-order walk of the tree of `+`)."""
    out = []

    def walk(start, n):
        if n <= PW_BLOCK:
            out.append([start, n, 0])
            return
        n2 = split(n)
        walk(start, n2)
        walk(start + n2, n - n2)
        out[-1][2] += 1

    walk(0, C)
    return [tuple(e) for e in out]


def sum_by_table(a: np.ndarray, table) -> np.ndarray:
    """The kernel's evaluation order: every leaf by `pairwise_sum`, then the stack walk the `adds` column describes."""
    stack = []
    for start, n, adds in table:
        v = pairwise_sum(np.ascontiguousarray(a[:, start:start + n]))
        for _ in range(adds):
            v = stack.pop() + v
        stack.append(v)
    assert len(stack) == 1
    return stack[0]


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
