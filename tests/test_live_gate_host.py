"""Host tests of the live frames' motion gate: the numpy model the GPU tests compare with (tests/_live_gate_ref.py) against a
scalar per-byte loop, MotionGate / resolve_motion_gate and every refusal, live.gate_decision on scripted {still, epoch}
sequences against the model's own wording of the rule, and the two entry points' refusals before any launch."""
import itertools
import math

import numpy as np
import pytest

from _live_gate_ref import (INIT, MotionGateRef, anchor_with_room, changed_bytes, changed_bytes_scalar, decision, frame_off_by,
                            off_positions)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0, 1, 7, 254, 255])
def test_the_count_is_the_scalar_loop(tau):
    rng = np.random.default_rng(tau)
    for shape in ((2, 3, 3), (1, 1, 3), (3, 5, 3)):
        for _ in range(20):
            f, a = (rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(2))
            assert changed_bytes(f, a, tau) == changed_bytes_scalar(f, a, tau)
    # the edges of a byte in both signs (uint8 arithmetic would wrap here), and |d| == tau in both signs, which is not changed
    f, a = np.array([0, 255, 0, 255, tau, 0], dtype=np.uint8), np.array([255, 0, 0, 255, 0, tau], dtype=np.uint8)
    assert changed_bytes(f, a, tau) == changed_bytes_scalar(f, a, tau) == (2 if tau < 255 else 0)
    if tau < 255:
        f[4:] = tau + 1, 0
        a[4:] = 0, tau + 1
        assert changed_bytes(f, a, tau) == changed_bytes_scalar(f, a, tau) == 4


def test_the_model_follows_the_rule_step_by_step():
    shape, tau, limit = (2, 2, 3), 3, 2
    rng = np.random.default_rng(5)
    a, b = MotionGateRef(3, shape, tau, limit), MotionGateRef(3, shape, tau, limit)
    assert a.state.tolist() == [list(INIT)] * 3
    base = anchor_with_room(rng, shape, tau + 1)
    fb = base.size
    steps = [([1], base),                                                        # no anchor: moves, changed -1
             ([1], frame_off_by(base, off_positions(fb, fb, 1, 2), tau + 1)),    # limit bytes above tau: still, changed 2, peak 2
             ([1], frame_off_by(base, off_positions(fb, fb, 1, fb), tau)),       # every byte off by exactly tau: still, changed 0
             ([1], frame_off_by(base, off_positions(fb, fb, 1, 3), tau + 1)),    # limit + 1: moves, changed 3, peak 0
             ([1, 7, -1], base)]                                                 # against the new anchor: 3 bytes back -> moves again
    want = [[0, 1, -1, 0], [1, 1, 2, 2], [2, 1, 0, 2], [0, 2, 3, 0], [0, 3, 3, 0]]
    for (cams, f), row in zip(steps, want):
        frames = np.stack([f] * len(cams))
        va = a.push(cams, frames)
        vb = b.push(cams, frames, count=changed_bytes_scalar)
        assert va == vb and a.state[1].tolist() == b.state[1].tolist() == row
        assert va[0] == (row[0] == 0) and va[1:] == [None] * (len(cams) - 1)
    assert np.array_equal(a.anchor[1], base) and np.array_equal(a.anchor, b.anchor)
    assert a.state[[0, 2]].tolist() == [list(INIT)] * 2 and not a.anchor[[0, 2]].any()
    a.state[1, 0] = (1 << 30) - 1  # still saturates
    a.push([1], base[None])
    a.push([1], base[None])
    assert a.state[1, 0] == 1 << 30
    a.reset([1])
    assert a.state[1].tolist() == [-1, 4, 0, 0] and a.push([1], base[None]) == [True] and a.state[1].tolist() == [0, 5, -1, 0]


# ---- MotionGate and resolve_motion_gate -----------------------------------------------------------------------------------------------
def test_motion_gate_resolution_and_limit():
    from anomaly_detection_on_video_amd.live import MotionGate, resolve_motion_gate

    assert resolve_motion_gate(None) is None
    g = MotionGate(6, 100)
    assert resolve_motion_gate(g) is g and (g.pixel_delta, g.max_changed, g.max_hold) == (6, 100, None)
    assert resolve_motion_gate({"pixel_delta": 6, "max_changed": 100}) == g == resolve_motion_gate((6, 100)) == resolve_motion_gate([6, 100, None])
    assert resolve_motion_gate({"pixel_delta": np.int64(0), "max_changed": np.float32(0.5), "max_hold": np.int32(3)}) == MotionGate(0, 0.5, 3)
    assert resolve_motion_gate((255, 0, 1)) == MotionGate(255, 0, max_hold=1)
    fb = 256 * 340 * 3
    for mc, want in ((0, 0), (1, 1), (fb, fb), (fb + 5, fb), (0.0, 0), (1.0, fb), (0.5, fb // 2), (0.001, 261), (1e-9, 0), (0.1, math.floor(0.1 * fb))):
        assert MotionGate(1, mc).limit(fb) == want, mc
    assert MotionGate(1, 0.34).limit(3) == 1 and MotionGate(1, 0.33).limit(3) == 0  # floor, not round
    with pytest.raises(TypeError):  # no defaults: nobody has measured what suits a real camera
        MotionGate()
    with pytest.raises(TypeError):
        MotionGate(6)
    assert "NO defaults" in MotionGate.__doc__


def test_motion_gate_refusals_name_the_field():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveFrames, MotionGate, resolve_motion_gate

    cases = [((-1, 0), "pixel_delta=-1 outside"), ((256, 0), "pixel_delta=256 outside"), ((1.0, 0), "pixel_delta=1.0 is not an integer"),
             ((True, 0), "pixel_delta=True is not an integer"), (("3", 0), "pixel_delta='3' is not an integer"),
             ((1, -1), "max_changed=-1 is negative"), ((1, -0.5), "max_changed=-0.5 is negative"), ((1, float("nan")), "max_changed=nan is not finite"),
             ((1, float("inf")), "max_changed=inf is not finite"), ((1, 1.5), "max_changed=1.5 is a share above 1"),
             ((1, True), "max_changed=True is neither"), ((1, "0.1"), "max_changed='0.1' is neither"), ((1, None), "max_changed=None is neither"),
             ((1, 0, 0), "max_hold=0 is below 1"), ((1, 0, -2), "max_hold=-2 is below 1"), ((1, 0, 1.0), "max_hold=1.0 is neither None nor an integer"),
             ((1, 0, True), "max_hold=True is neither None nor an integer")]
    for args, what in cases:
        with pytest.raises(ValueError, match="motion: " + what):
            MotionGate(*args)
        with pytest.raises(ValueError, match="motion: " + what):
            resolve_motion_gate(args)
        with pytest.raises(ValueError, match="motion: " + what):
            resolve_motion_gate(dict(zip(("pixel_delta", "max_changed", "max_hold"), args)))
        with pytest.raises(HipExtensionError, match="LiveFrames: motion: " + what):  # refused before the device is looked at
            LiveFrames(2, motion=args, device="cpu")
    for spec, what in ((5, "expected a mapping, a tuple or a MotionGate, got int"), ("gate", "expected a mapping, a tuple or a MotionGate, got str"),
                       ((1,), r"a tuple holds \(pixel_delta, max_changed\[, max_hold\]\), got 1 values"), ((1, 2, 3, 4), r"a tuple holds .*, got 4 values"),
                       ({"pixel_delta": 1}, "max_changed is missing"), ({"max_changed": 1}, "pixel_delta is missing"),
                       ({"pixel_delta": 1, "max_changed": 1, "tau": 2}, r"unknown key\(s\) \['tau'\]")):
        with pytest.raises(ValueError, match="motion: " + what):
            resolve_motion_gate(spec)
    with pytest.raises(HipExtensionError, match="LiveFrames: device 'cpu': the rings live on the GPU"):
        LiveFrames(2, motion=(1, 0), device="cpu")  # a good gate: the next refusal is the device's
    with pytest.raises(HipExtensionError, match=r"LiveFrames: frames of 3221225472 bytes: the motion gate counts changed bytes in int32"):
        LiveFrames(1, frame_hw=(32768, 32768), frames_per_clip=1, motion=(0, 0), device="cpu")
    with pytest.raises(HipExtensionError, match="LiveFrames: device 'cpu'"):
        LiveFrames(1, frame_hw=(32768, 32768), frames_per_clip=1, device="cpu")  # (the rings themselves have no such bound)


# ---- gate_decision -----------------------------------------------------------------------------------------------------------------------
def _run(seq, span, max_hold, fn):
    """seq: [(still, epoch)] at a camera's successive due windows -> the decisions as a string of E / H."""
    ref, holds, out = None, 0, ""
    for still, epoch in seq:
        held, ref, holds = fn(still, epoch, span, ref, holds, max_hold)
        out += "H" if held else "E"
    return out


def test_gate_decision_on_scripted_sequences():
    from anomaly_detection_on_video_amd.live import gate_decision

    span = 16
    cases = [
        # a camera that never rests: every window is extracted
        ([(0, 16), (0, 24), (3, 30), (14, 31)], None, "EEEE"),
        # still from its first frame, one window every 8 frames: the first quiet window is the reference, the rest repeat it
        ([(15, 1), (23, 1), (31, 1), (39, 1), (47, 1)], None, "EHHHH"),
        ([(15, 1), (23, 1), (31, 1), (39, 1), (47, 1)], 2, "EHHEH"),
        ([(15, 1), (23, 1), (31, 1), (39, 1), (47, 1), (55, 1), (63, 1)], 1, "EHEHEHE"),
        # still + 1 == span is quiet, still + 1 == span - 1 is not
        ([(14, 1), (15, 2), (15, 2)], None, "EEH"),
        # motion between two quiet stretches: the first quiet window under the new anchor is extracted again
        ([(15, 1), (23, 1), (3, 2), (11, 2), (19, 2), (27, 2)], None, "EHEEEH"),
        # a new anchor under which the camera is quiet at once at the next window (epoch moved): never held across epochs
        ([(20, 1), (28, 1), (15, 2), (23, 2)], None, "EHEH"),
        # the scene change of the end-to-end test: anchor at frame 20, windows end at frames 15, 23, 31, 39, 47
        ([(15, 1), (3, 2), (11, 2), (19, 2), (27, 2)], None, "EEEEH"),
        # the saturated counter is still quiet
        ([(1 << 30, 7), (1 << 30, 7)], None, "EH"),
    ]
    for seq, max_hold, want in cases:
        assert _run(seq, span, max_hold, gate_decision) == want, (seq, max_hold)
        assert _run(seq, span, max_hold, decision) == want, (seq, max_hold)  # the model says the same
    assert _run([(0, 1), (0, 1), (0, 2)], 1, None, gate_decision) == "EHE"  # span 1: every frame is a window


def test_gate_decision_equals_the_model_on_every_short_sequence():
    from anomaly_detection_on_video_amd.live import gate_decision

    span = 4
    moves = [(2, 1), (3, 1), (7, 1), (0, 2), (3, 2), (5, 2), (3, 3)]
    for max_hold in (None, 1, 2):
        for seq in itertools.product(moves, repeat=4):
            ref_a = ref_b = None
            holds_a = holds_b = 0
            for still, epoch in seq:
                got = gate_decision(still, epoch, span, ref_a, holds_a, max_hold)
                want = decision(still, epoch, span, ref_b, holds_b, max_hold)
                assert got == want, (seq, max_hold)
                (_, ref_a, holds_a), (_, ref_b, holds_b) = got, want


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_null_pointers_and_bad_sizes_before_any_launch():
    """Pure host-side validation: every call returns ADVHIP_EINVAL with a message, with or without a GPU."""
    import __graft_entry__
    from anomaly_detection_on_video_amd import _lib

    __graft_entry__.build()
    lib = _lib.load()
    assert lib.advhip_abi_version() == 2  # additions only
    p = 4096  # never dereferenced: every call below is refused first
    gate, rep = lib.advhip_frame_gate_update_u8, lib.advhip_ring_repeat_f32
    cases = [
        (gate, (None, p, p, p, p, 1, 1, 48, 3, 5, None), "frame_gate_update: null pointer"),
        (gate, (p, None, p, p, p, 1, 1, 48, 3, 5, None), "frame_gate_update: null pointer"),
        (gate, (p, p, None, p, p, 1, 1, 48, 3, 5, None), "frame_gate_update: null pointer"),
        (gate, (p, p, p, None, p, 1, 1, 48, 3, 5, None), "frame_gate_update: null pointer"),
        (gate, (p, p, p, p, None, 1, 1, 48, 3, 5, None), "frame_gate_update: null pointer"),
        (gate, (p, p, p, p, p, 0, 1, 48, 3, 5, None), "frame_gate_update: bad shape"),
        (gate, (p, p, p, p, p, 1, 0, 48, 3, 5, None), "frame_gate_update: bad shape"),
        (gate, (p, p, p, p, p, 1, 1, 0, 3, 0, None), "frame_gate_update: bad shape"),
        (gate, (p, p, p, p, p, 1, 1, 1 << 31, 3, 5, None), "frame_gate_update: bad shape"),
        (gate, (p, p, p, p, p, 3, 2, 48, 3, 5, None), "frame_gate_update: 3 frames for 2 cameras"),
        (gate, (p, p, p, p, p, 1, 1, 48, -1, 5, None), "frame_gate_update: pixel_delta -1 outside [0, 255]"),
        (gate, (p, p, p, p, p, 1, 1, 48, 256, 5, None), "frame_gate_update: pixel_delta 256 outside [0, 255]"),
        (gate, (p, p, p, p, p, 1, 1, 48, 3, -1, None), "frame_gate_update: limit -1 outside [0, frame_bytes = 48]"),
        (gate, (p, p, p, p, p, 1, 1, 48, 3, 49, None), "frame_gate_update: limit 49 outside [0, frame_bytes = 48]"),
        (gate, (p, p, p, p, p, 65536, 70000, 48, 3, 5, None), "frame_gate_update: 65536 rows of 48 bytes are outside the launch grid"),
        (rep, (None, p, p, 1, 1, 1, 4, 9, None), "ring_repeat: null pointer"),
        (rep, (p, None, p, 1, 1, 1, 4, 9, None), "ring_repeat: null pointer"),
        (rep, (p, p, None, 1, 1, 1, 4, 9, None), "ring_repeat: null pointer"),
        (rep, (p, p, p, 0, 1, 1, 4, 9, None), "ring_repeat: bad shape"),
        (rep, (p, p, p, 1, 0, 1, 4, 9, None), "ring_repeat: bad shape"),
        (rep, (p, p, p, 1, 1, 0, 4, 9, None), "ring_repeat: bad shape"),
        (rep, (p, p, p, 1, 1, 1, 0, 9, None), "ring_repeat: bad shape"),
        (rep, (p, p, p, 1, 1, 1, 4, 0, None), "ring_repeat: bad shape"),
        (rep, (p, p, p, 1 << 30, 1, 2, 4, 9, None), "ring_repeat: 2147483648 rows is outside the launch grid"),
    ]
    for fn, args, what in cases:
        assert fn(*args) == -1 and what in lib.advhip_last_error().decode(), (what, lib.advhip_last_error())
