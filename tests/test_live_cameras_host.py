"""Host tests of live.CameraSet, built on "cpu": the one rule for the `cams` of a call with every refusal text for each owner's
unit, the cache of id vectors (a repeated tuple's tensor is reused, the least recently used of more than 64 goes), and the host
mirror of the counts, which only `bump` and `clear` move and only for the listed cameras."""
import re

import numpy as np
import pytest
import torch

UNITS = ("frame", "clip", "sample")

REFUSALS = (
    ([1, 1], "duplicate camera ids [1]: one {unit} per camera and call"),
    ([0, 4], "camera id 4 is out of range [0, 4)"),
    ([-1, 0], "camera id -1 is out of range [0, 4)"),
    ([], "an empty list of cameras"),
    ((), "an empty list of cameras"),
    ([0, 1.5], "camera id 1.5 is not a host integer"),
    ([0, "1"], "camera id '1' is not a host integer"),
    (torch.tensor([0, 1]), "cams must be a sequence of host integers, got a Tensor"),
    (np.array([0, 1]), "cams must be a sequence of host integers, got a ndarray"),
    (3, "cams must be a sequence of camera ids, got int"),
    ([0, True], "camera id True is not a host integer"),
)


@pytest.mark.parametrize("unit", UNITS)
def test_check_refuses_with_the_stated_texts(unit):
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import CameraSet

    cs = CameraSet(4, "cpu", unit)
    assert cs.n_cameras == 4 and cs.device == torch.device("cpu")
    for cams, what in REFUSALS:
        with pytest.raises(HipExtensionError, match=re.escape(f"Owner.call: {what.format(unit=unit)}")):
            cs.check(cams, "Owner.call")
    assert not cs.ids.items and cs.host == [0] * 4  # a refusal caches nothing and counts nothing
    assert cs.check([3, np.int64(0), 2.0], "x") == (3, 0, 2) and all(type(c) is int for c in cs.check([np.int32(1), 2.0], "x"))
    assert cs.check(range(4), "x") == (0, 1, 2, 3)


def test_a_repeated_tuple_keeps_its_tensor_and_the_least_recently_used_of_65_goes():
    from anomaly_detection_on_video_amd.live import CACHE_ENTRIES, CameraSet

    assert CACHE_ENTRIES == 64
    cs = CameraSet(70, "cpu", "clip")
    first = cs.check((0, 1), "x")
    ids = cs.ids(first)
    assert ids.dtype == torch.int32 and ids.tolist() == [0, 1]
    assert cs.check(first, "x") is first and cs.check((0, 1), "x") == first == cs.check([0, 1], "x")  # (a cache key returns at once)
    assert cs.ids((0, 1)) is ids and cs.ids(cs.check([0, 1], "x")) is ids
    kept = cs.ids(cs.check((1, 0), "x"))                      # the second entry: another order is another vector
    assert kept.tolist() == [1, 0]
    others = [(c, c + 1) for c in range(2, 64)]               # 62 more: the cache is full
    for t in others:
        cs.ids(cs.check(t, "x"))
    assert len(cs.ids.items) == 64 and cs.ids((0, 1)) is ids  # (touched: now the most recently used; (1, 0) is the oldest)
    cs.ids(cs.check((68, 69), "x"))                           # the 65th distinct tuple
    assert len(cs.ids.items) == 64 and (1, 0) not in cs.ids.items and (0, 1) in cs.ids.items
    assert cs.ids((0, 1)) is ids                              # touched before the 65th: it survived
    again = cs.ids(cs.check((1, 0), "x"))
    assert again is not kept and again.tolist() == [1, 0]     # evicted: a new tensor


def test_an_untouched_first_tuple_is_evicted_by_the_65th():
    from anomaly_detection_on_video_amd.live import CameraSet

    cs = CameraSet(70, "cpu", "frame")
    ids = cs.ids(cs.check((0, 1), "x"))
    for c in range(2, 66):  # 64 more distinct tuples
        cs.ids(cs.check((c, c + 1), "x"))
    assert (0, 1) not in cs.ids.items and len(cs.ids.items) == 64
    new = cs.ids(cs.check((0, 1), "x"))
    assert new is not ids and torch.equal(new, ids)


def test_bump_and_clear_move_only_the_listed_cameras():
    from anomaly_detection_on_video_amd.live import CameraSet

    cs = CameraSet(4, "cpu", "sample")
    cs.bump((0, 2))
    cs.bump((2, 3))
    assert cs.host == [1, 0, 2, 1]
    cs.clear((2,))
    assert cs.host == [1, 0, 0, 1]
    cs.bump((1,))
    cs.clear((0, 3))
    assert cs.host == [0, 1, 0, 0]


def test_sharing_is_of_the_id_cache_only_and_only_among_the_same_cameras():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import CameraSet

    a = CameraSet(4, "cpu", "clip")
    b = CameraSet(4, "cpu", "sample", share=a)
    ids = a.ids(a.check([0, 2], "x"))
    assert b.check((0, 2), "x") == (0, 2) and b.ids((0, 2)) is ids
    a.bump((0, 2))
    assert a.host == [1, 0, 1, 0] and b.host == [0] * 4
    with pytest.raises(HipExtensionError, match=r"duplicate camera ids \[1\]: one sample per camera and call"):
        b.check([1, 1], "x")
    with pytest.raises(HipExtensionError, match="CameraSet: 4 cameras on cpu share no ids with 5 on cpu"):
        CameraSet(5, "cpu", "sample", share=a)
