"""The occlusion-aware video mask propagate from several keyframes, the parts that need no device: the restatement
(tests/propagate_keys_visible_ref.py) checked on its own -- what the rule promises, as bits, an empty key, and the quality
conditions on a disc that passes behind a bar with a key on either side --, the three C entries' argument checks (made before any
HIP call), the wrapper's refusals, the node's protocol, and that the existing propagate nodes are as they were.  Layouts,
constants and names against the header are tests/test_cabi_mirror.py's, for the whole C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi
from tests import propagate_keys_ref as kref
from tests import propagate_keys_visible_ref as kvref
from tests import propagate_ref as ref
from tests import propagate_visible_ref as vref
from tests.compare import _f32_bits as _bits, _iou
from tests.propagate_scenes import _moving, _moving_disc as _disc, _texture, occluded_disc_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS, SEARCH, SMOOTH = 3, 2, 8


# ---- what follows from the rule, on the restatement alone -------------------------------------------------------------------------------
def test_one_key_is_the_single_key_form_and_occlusion_zero_is_the_keys_form():
    H, W, F = 23, 33, 5
    video = _moving(F, H, W)
    soft = np.random.default_rng(2).random((H, W), dtype=np.float32)
    for key in (0, 2, 4):
        mask, hidden = kvref.propagate_keys_visible_ref(video, soft[None], [key], LEVELS, SEARCH, SMOOTH, 16)
        want, want_hidden = vref.propagate_visible_ref(video, soft, key, LEVELS, SEARCH, SMOOTH, 16)
        assert (_bits(mask) == _bits(want)).all() and (_bits(hidden) == _bits(want_hidden)).all(), key
    masks = np.stack([soft, _disc(H, W, 11, 16, 7)])
    mask, hidden = kvref.propagate_keys_visible_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH, 0)
    assert (_bits(mask) == _bits(kref.propagate_keys_ref(video, masks, [1, 4], LEVELS, SEARCH, SMOOTH))).all()
    assert (_bits(hidden) == 0).all()


def test_a_still_video_empty_keys_the_keys_themselves_and_the_codes():
    rng = np.random.default_rng(3)
    H, W, F = 23, 33, 6
    soft = rng.random((H, W), dtype=np.float32)
    binar = ref.binarise(soft).astype(np.float32)
    still = np.repeat(rng.random((1, H, W, 3), dtype=np.float32), F, axis=0)
    for keys in ([0, 5], [1, 3, 4], [2]):
        for occlusion in (1, 16, 255):
            mask, hidden = kvref.propagate_keys_visible_ref(still, np.repeat(soft[None], len(keys), axis=0), keys, LEVELS, SEARCH, SMOOTH, occlusion)
            assert mask.dtype == hidden.dtype == np.float32
            assert (_bits(mask) == _bits(np.repeat(binar[None], F, axis=0))).all() and (_bits(hidden) == 0).all(), (keys, occlusion)
    video = _moving(F, H, W)
    mask, hidden = kvref.propagate_keys_visible_ref(video, np.zeros((3, H, W), np.float32), [0, 3, 5], LEVELS, SEARCH, SMOOTH, 1)
    assert (_bits(mask) == 0).all() and (_bits(hidden) == 0).all()
    # on every key the painting; mask + hidden a multiple of 1 / 256 everywhere, at a threshold that flags a lot
    masks = np.stack([_disc(H, W, 11, 10, 7), soft, _disc(H, W, 12, 20, 6)])
    for occlusion in (1, 16):
        mask, hidden = kvref.propagate_keys_visible_ref(video, masks, [0, 3, 5], LEVELS, SEARCH, SMOOTH, occlusion)
        for i, k in enumerate((0, 3, 5)):
            assert (_bits(mask[k]) == _bits(ref.binarise(masks[i]).astype(np.float32))).all() and (_bits(hidden[k]) == 0).all()
        total = (mask.astype(np.float64) + hidden.astype(np.float64)) * 256
        assert (total == np.round(total)).all() and total.min() >= 0 and total.max() <= 256
        assert (mask >= 0).all() and (hidden >= 0).all()
        assert occlusion != 1 or hidden.sum() > 0


def test_the_pieces_of_the_rule_one_at_a_time():
    assert not kvref.lost_at([100, 50, 16, 16], 3) and kvref.lost_at([100, 50, 15, 200], 2) and kvref.lost_at([100, 50, 15, 200], 3)
    assert not kvref.lost_at([100, 50, 15, 200], 1) and not kvref.lost_at([100, 0, 0], 0)
    assert kvref.lost_at([16, 15], 1) and not kvref.lost_at([15, 0, 0], 2) and not kvref.lost_at([0, 0, 0], 2)       # a key below 16 bits
    assert ref.MIN_PIXELS == _cabi.LP_PROP_MIN_PIXELS == 16
    H, W = 16, 24
    inside = np.full((H, W), 4096, np.int64)
    assert (kvref.merged_code(inside, inside, 5, 2) == 256).all() and (kvref.merged_code(-inside, -inside, 5, 2) == 0).all()
    # a pixel at distance 1 inside in A and 1 outside in B: S = 0.5 + ((n - j) - j) / n, in codes of 1 / 256, rounded half up
    one = np.ones((1, 1), np.int64)
    assert kvref.merged_code(one, -one, 4, 2)[0, 0] == 128 and kvref.merged_code(one, -one, 8, 3)[0, 0] == 192
    assert kvref.merged_code(one, -one, 3, 1)[0, 0] == int(np.float32(np.float32(0.5 + 1 / 3) * np.float32(256)) + np.float32(0.5))
    # exactly one lost: the other chain, bit for bit; none or both: the merged code split by the nearer key's flags
    rng = np.random.default_rng(4)
    cA, cB = rng.integers(0, 257, (H, W)), rng.integers(0, 257, (H, W))
    fA, fB = np.zeros((2, 3), np.int64), np.ones((2, 3), np.int64)
    A, B = (cA, vref.occlude(cA, fB), fB), (cB, vref.occlude(cB, fA), fA)
    qa, qb = kvref.subject_q(cA), kvref.subject_q(cB)
    for lost, want in (((True, False), B), ((False, True), A)):
        mask, hidden = kvref.merge_frame(qa, qb, A, B, *lost, 4, 1)
        assert ((mask * 256).astype(np.int64) == want[1]).all() and ((hidden * 256).astype(np.int64) == want[0] - want[1]).all()
    cs = kvref.merged_code(qa, qb, 4, 2)
    for lost in ((False, False), (True, True)):
        mask, hidden = kvref.merge_frame(qa, qb, A, B, *lost, 4, 2)                  # 2 j <= n: A's flags, all occluded here
        assert not mask.any() and ((hidden * 256).astype(np.int64) == cs).all()
        mask, hidden = kvref.merge_frame(qa, qb, A, B, *lost, 4, 3)                  # B's flags: nothing occluded
        assert not hidden.any() and ((mask * 256).astype(np.int64) == kvref.merged_code(qa, qb, 4, 3)).all()


def test_an_empty_key_is_never_lost_and_the_subject_is_the_keys_merge_of_the_same_codes():
    """No occluder in the picture, a disc on key 0 and nothing on key 8: the empty key's chain has a count of 0 everywhere and is
    never lost, the disc's chain is not lost either, so every in-between frame is the merge.  Fed the same chains' codes,
    propagate_keys_ref gives S; the subject here is S rounded to a code.  (The empty key's distance is the cap, 64: the disc of
    depth 12 shows only where 7 * 12 > 64, on the first frame.)"""
    F, H, W = 9, 40, 56
    canvas = _texture(np.random.default_rng(6), 64, 128).astype(np.float32)[..., None]
    video = np.stack([canvas[t:t + H, 2 * t:2 * t + W] for t in range(F)])
    masks = np.stack([_disc(H, W, 20, 32, 12), np.zeros((H, W), np.float32)])
    trace = {}
    mask, hidden = kvref.propagate_keys_visible_ref(video, masks, [0, 8], LEVELS, SEARCH, SMOOTH, 16, trace)
    chains = trace["chains"]
    assert chains[(1, -1)][1] == [0] * 8 and chains[(0, 1)][1][0] >= 16
    assert trace["lost"] == {t: (False, False) for t in range(1, 8)}
    codes = {key: {t: c.astype(np.float32) / np.float32(256) for t, (c, _, _) in frames.items()} for key, (frames, _) in chains.items()}
    S = kref.propagate_keys_ref(video, masks, [0, 8], LEVELS, SEARCH, SMOOTH, chain=lambda i, k, d, length: codes[(i, d)])
    subject = ((mask + hidden) * np.float32(256)).astype(np.int64)
    want = ((S * np.float32(256)).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int64)
    assert (subject[1:8] == want[1:8]).all() and subject[1].any() and not (_bits(mask[8]) | _bits(hidden[8])).any()
    # an empty key next to a chain that does get lost: that frame is the empty chain's, nothing
    frames, counts = chains[(0, 1)]
    assert kvref.lost_at([counts[0], 3, 3, 3], 1) and not kvref.lost_at(chains[(1, -1)][1], 7)
    A, B = frames[1], chains[(1, -1)][0][1]
    m, h = kvref.merge_frame(kvref.subject_q(A[0]), kvref.subject_q(B[0]), A, B, True, False, 8, 1)
    assert not m.any() and not h.any()


# ---- the quality conditions, on the restatement alone ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _quality():
    images, discs, on_bar = occluded_disc_clip(seed=0, F=16, H=64, W=96, radius=12, bar=(28, 44))
    masks = np.stack([discs[0], discs[15]]).astype(np.float32)
    trace = {}
    mask, hidden = kvref.propagate_keys_visible_ref(images, masks, [0, 15], LEVELS, SEARCH, SMOOTH, 16, trace)
    plain = kref.propagate_keys_ref(images, masks, [0, 15], LEVELS, SEARCH, SMOOTH)
    return images, discs, on_bar, mask, hidden, plain, trace


def test_a_disc_behind_a_bar_with_a_key_on_either_side():
    """64 x 96, 16 frames, a disc of radius 12 that passes behind a bar of 16 px, keys on frames 0 and 15, levels 3, occlusion 16;
    the subject is mask + hidden >= 0.5 against the whole disc over frames 1..14.  Measured on the restatement: (a) mean IoU 0.967
    (min 0.921) against 0.304 for propagate_keys_ref; (b) the forward chain is lost from frame 7 on, the backward chain on frames
    1..7, exactly one chain on 13 of the 14 frames; (c) hidden >= 0.5 has 2150 px on the bar and 887 off it; (d) mask >= 0.5 puts
    30 px on the bar against 111 for propagate_keys_ref."""
    _, discs, on_bar, mask, hidden, plain, trace = _quality()
    mid = range(1, 15)
    iou = [_iou((mask[t] + hidden[t]) >= 0.5, discs[t]) for t in mid]
    iou_plain = [_iou(plain[t] >= 0.5, discs[t]) for t in mid]
    lost_a, lost_b = [trace["lost"][t][0] for t in mid], [trace["lost"][t][1] for t in mid]
    hid = hidden >= 0.5
    on, off = sum(int((hid[t] & on_bar).sum()) for t in mid), sum(int((hid[t] & ~on_bar).sum()) for t in mid)
    leak, leak_plain = (sum(int(((m[t] >= 0.5) & on_bar).sum()) for t in mid) for m in (mask, plain))
    print({"iou": (np.mean(iou), min(iou)), "iou_plain": np.mean(iou_plain), "lost_a": lost_a, "lost_b": lost_b, "hidden": (on, off),
           "leak": (leak, leak_plain)})
    assert np.mean(iou) >= 0.8 and np.mean(iou) >= 2 * np.mean(iou_plain)                                            # (a)
    first_a, last_b = lost_a.index(True), len(lost_b) - 1 - lost_b[::-1].index(True)
    assert all(lost_a[first_a:]) and not any(lost_a[:first_a]) and all(lost_b[:last_b + 1]) and not any(lost_b[last_b + 1:])   # (b)
    assert any(a != b for a, b in zip(lost_a, lost_b))
    assert on > off                                                                                                  # (c)
    assert 2 * leak <= leak_plain                                                                                    # (d)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_batch_entries_and_the_merge_reject_bad_arguments_without_a_device(hip_lib):
    C, E = ctypes, _cabi.LP_E_INVALID
    p = [256 << k for k in range(12)]                                   # never dereferenced: validation comes before any HIP call
    side = _cabi.LP_VMASK_MAX_SIDE

    def visible(jobs=1, job=None, table=True, **kw):
        rows = (_cabi.LpPropVisibleJob * max(jobs, 1))(*[_cabi.LpPropVisibleJob(**{**dict(pos=p[0], tgt=p[1], key=p[2], mask=p[3], flags=p[4]),
                                                                                  **(job or {})}) for _ in range(max(jobs, 1))])
        d = dict(height=40, width=70, occlusion=16, jobs=jobs, job=C.addressof(rows) if table else None)
        return hip_lib.lp_prop_visible_batch(C.byref(_cabi.LpPropVisibleBatchDesc(**{**d, **kw})), None)
    assert hip_lib.lp_prop_visible_batch(None, None) == E
    for kw in (dict(jobs=0), dict(jobs=33), dict(jobs=-1), dict(table=False), dict(height=0), dict(height=side + 1), dict(width=0),
               dict(width=side + 1), dict(occlusion=0), dict(occlusion=256), *[dict(job={f: None}) for f in ("pos", "tgt", "key", "mask", "flags")],
               *[dict(job={"flags": p[k]}) for k in range(4)], dict(jobs=32, job={"key": None})):
        assert visible(**kw) == E, kw

    def occlude(jobs=1, job=None, table=True, **kw):
        good = dict(code=p[0], flags=p[1], out=p[2], hidden=p[3], mask_pyramid=p[4], count=p[5])
        rows = (_cabi.LpPropOccludeJob * max(jobs, 1))(*[_cabi.LpPropOccludeJob(**{**good, **(job or {})}) for _ in range(max(jobs, 1))])
        d = dict(height=40, width=70, levels=3, jobs=jobs, job=C.addressof(rows) if table else None)
        return hip_lib.lp_prop_occlude_batch(C.byref(_cabi.LpPropOccludeBatchDesc(**{**d, **kw})), None)
    assert hip_lib.lp_prop_occlude_batch(None, None) == E
    for kw in (dict(jobs=0), dict(jobs=33), dict(table=False), dict(height=0), dict(height=side + 1), dict(width=0), dict(width=side + 1),
               dict(levels=0), dict(levels=7), *[dict(job={f: None}) for f in ("code", "flags", "out", "hidden", "mask_pyramid")],
               *[dict(job={f: p[k]}) for f, ks in (("out", (0, 1)), ("hidden", (0, 1, 2)), ("mask_pyramid", (0, 1, 2, 3)), ("count", (0, 1, 2, 3, 4)))
                 for k in ks], dict(jobs=32, job={"out": None})):
        assert occlude(**kw) == E, kw

    good = dict(frames=3, height=40, width=70, span=4, first=1, qa=p[0], qb=p[1], code_a=p[2], mask_a=p[3], code_b=p[4], mask_b=p[5],
                flags_a=p[6], flags_b=p[7], count_a=p[8], count_b=p[9], out=p[10], hidden=p[11])
    inputs = ("qa", "qb", "code_a", "mask_a", "code_b", "mask_b", "flags_a", "flags_b", "count_a", "count_b")
    assert hip_lib.lp_prop_merge_visible(None, None) == E
    for change in ({"height": 0}, {"height": side + 1}, {"width": 0}, {"width": side + 1}, {"span": 1}, {"first": 0}, {"frames": 0},
                   {"frames": 4}, {"first": 2}, *[{f: None} for f in inputs + ("out", "hidden")], {"out": p[11]},
                   *[{"out": good[f]} for f in inputs if f != "mask_a"], *[{"hidden": good[f]} for f in inputs if f != "code_a"]):
        assert hip_lib.lp_prop_merge_visible(C.byref(_cabi.LpPropMergeVisibleDesc(**{**good, **change})), None) == E, change
    too_long = {**good, "span": 65536}
    assert hip_lib.lp_prop_merge_visible(C.byref(_cabi.LpPropMergeVisibleDesc(**too_long)), None) == _cabi.LP_E_UNSUPPORTED


def test_the_header_says_the_keys_visible_words():
    header = open(os.path.join(ROOT, "include", "lanpaint_hip.h")).read()
    for word in ("exactly one of A, B lost at t", "c_S = (int)(S * 256.0f + 0.5f)", "f = f_A if 2 j <= n, else f_B", "never lost",
                 "c'_S = (c_S * w + 128) >> 8", "Lost is sticky", "one integer atomic add per wave"):
        assert word in header, word


# ---- the wrapper and the node ---------------------------------------------------------------------------------------------------------
def test_propagate_keys_visible_refuses_cpu_tensors_and_bad_arguments():
    from lanpaint_amd import propagate_keys_visible as kv
    images, masks = torch.zeros(4, 16, 16, 3), torch.zeros(2, 16, 16)
    u8, i32 = torch.zeros(16, 16, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32)
    for call in (lambda: kv.propagate_keys_visible(images, masks, [0, 3]), lambda: kv.propagate_keys_visible(images, masks, [0, 3], occlusion=0),
                 lambda: kv.visible_flags_batch([(torch.zeros(16, 16, 2, dtype=torch.int32), u8, u8, u8)]),
                 lambda: kv.occlude_batch([(torch.zeros(16, 16), i32)], 3),
                 lambda: kv.merge_gap_visible(torch.zeros(1, 16, 16, dtype=torch.int32), *[None] * 9, span=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (dict(occlusion=-1), dict(occlusion=256), dict(occlusion=16.0), dict(occlusion=True), dict(levels=0), dict(search=8),
                dict(smooth=65)):
        with pytest.raises(ValueError):
            kv.propagate_keys_visible(images, masks, [0, 3], **bad)
    for bad_keys in ([3, 0], [0, 0], [0, 4], [-1], [], 3, [0.0]):        # the keys are looked at before any tensor's device
        with pytest.raises(ValueError):
            kv.propagate_keys_visible(images, masks, bad_keys)
    with pytest.raises(ValueError):
        kv.visible_flags_batch([], 0)
    with pytest.raises(ValueError):
        kv.merge_gap_visible(None, *[None] * 9, span=1)
    assert kv.DEFAULT_OCCLUSION == 16 and kv.MAX_OCCLUSION == 255 and kv.MAX_JOBS == 32 and kv.WS_CAP_BYTES == 1 << 30


def test_keys_visible_node_protocol_and_the_existing_propagate_nodes_are_untouched():
    from lanpaint_amd import propagate_keys_nodes, propagate_keys_visible_nodes, propagate_nodes, propagate_visible_nodes
    mod, name = propagate_keys_visible_nodes, "LanPaint_VideoMaskPropagateKeysVisible"
    node = mod.LanPaint_VideoMaskPropagateKeysVisible
    assert mod.NODE_CLASS_MAPPINGS == {name: node}
    assert mod.NODE_DISPLAY_NAME_MAPPINGS == {name: "LanPaint Video Mask Propagate (Keys, Visible)"}
    assert propagate_nodes.NODE_CLASS_MAPPINGS == {"LanPaint_VideoMaskPropagate": propagate_nodes.LanPaint_VideoMaskPropagate}
    assert list(propagate_keys_nodes.NODE_CLASS_MAPPINGS) == ["LanPaint_VideoMaskPropagateKeys"]
    assert list(propagate_visible_nodes.NODE_CLASS_MAPPINGS) == ["LanPaint_VideoMaskPropagateVisible"]
    keys_node, visible_node = propagate_keys_nodes.LanPaint_VideoMaskPropagateKeys, propagate_visible_nodes.LanPaint_VideoMaskPropagateVisible
    assert list(keys_node.INPUT_TYPES()["required"]) == ["image", "mask", "key_frames", "levels", "search", "smooth"]
    assert keys_node.RETURN_NAMES == ("mask",) and visible_node.RETURN_NAMES == ("mask", "hidden")
    assert list(visible_node.INPUT_TYPES()["required"]) == ["image", "mask", "key_frame", "levels", "search", "smooth", "occlusion"]
    types = node.INPUT_TYPES()
    req = types["required"]
    assert list(types) == ["required"] and list(req) == ["image", "mask", "key_frames", "levels", "search", "smooth", "occlusion"]
    for field, spec in keys_node.INPUT_TYPES()["required"].items():       # the inputs of the Keys node ...
        assert req[field] == spec, field
    assert req["occlusion"] == visible_node.INPUT_TYPES()["required"]["occlusion"]                      # ... plus occlusion
    assert req["occlusion"][0] == "INT" and req["occlusion"][1] == {**req["occlusion"][1], "default": 16, "min": 0, "max": 255}
    assert node.RETURN_TYPES == ("MASK", "MASK") and node.RETURN_NAMES == ("mask", "hidden") and len(node.OUTPUT_TOOLTIPS) == 2
    assert node.FUNCTION == "propagate" and node.CATEGORY == "mask" and callable(getattr(node, node.FUNCTION))
    for word in ("several key frames", "in front of the subject", "hidden", "second key behind the occluder", "stabilize", "mask refine",
                 "Detailer", "empty key"):
        assert word in node.DESCRIPTION, word
    with pytest.raises(ValueError):                                     # bad keys are refused before a device is looked for
        node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(2, 16, 16), "3, 0")
    with pytest.raises(ValueError):
        node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(2, 16, 16), "0, 4")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            node().propagate(torch.zeros(4, 16, 16, 3), torch.zeros(2, 16, 16), "0 3", 4, 2, 8, 16)
