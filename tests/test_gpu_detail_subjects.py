"""The per-subject Detailer on the MI355X (lanpaint_amd.detail_subjects, csrc/label_kernel.hip, csrc/detail_kernel.hip):
lp_mask_components_frames against scipy's 26-connected labelling (tests/subjects_ref.py), lp_subject_boxes against numpy,
lp_detail_resample_subjects and lp_detail_stitch_subjects bit for bit against the single-window entries called once per
(subject, frame) with erased masks built in torch from the label volume, the composed stitch against the torch restatement, and
the two nodes.  Every comparison covers every element."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

from lanpaint_amd import _cabi, detail, detail_color_nodes, detail_subject_nodes, detail_subjects, detail_track_nodes
from lanpaint_amd._util import raw_stream
from tests import detail_ref, subjects_ref
from tests.compare import _tensor_bits as _bits
from tests.device import DEV, _gen

pytestmark = pytest.mark.gpu
CAP = _cabi.LP_DETAIL_MAX_COMPONENTS


# ---- lp_mask_components_frames -----------------------------------------------------------------------------------------------------
def _check_components(mask, what):
    """mask: CPU tensor [F, H, W], or a HIP tensor to be used as it is (its alignment matters).  Labels (every voxel), count and
    table (every row below the cap) equal scipy's."""
    labels, n, table = detail_subjects.mask_components_frames(mask if mask.is_cuda else mask.to(DEV))
    want_labels, want_n, want_table = subjects_ref.label_frames_ref(mask.cpu().numpy() > 0.5)
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == tuple(mask.shape)
    assert n == want_n, (what, n, want_n)
    assert np.array_equal(labels.cpu().numpy(), want_labels), what
    assert len(table) == min(n, CAP) and np.array_equal(np.array(table, np.int64).reshape(-1, 7), want_table[:CAP]), what
    return labels, n, table


# (1, 20, 70), (5, 16, 64): n % 4 == 0, the 16 B path; (3, 17, 65), (2, 9, 7), (2, 1, 1): the scalar path.  All but the last two
# cross a 64-wide or a 16-high tile edge; (3, 17, 65) and (4, 33, 130) cross a 1024-element chunk edge.
@pytest.mark.parametrize("shape", [(1, 20, 70), (3, 17, 65), (4, 33, 130), (5, 16, 64), (2, 1, 1), (2, 9, 7)])
def test_components_frames_equal_scipy_on_random_volumes(shape):
    g = _gen(shape[-1] + shape[0])
    for density in (0.1, 0.3, 0.5):
        mask = (torch.rand(shape, generator=g) < density).float() * (0.45 + 0.55 * torch.rand(shape, generator=g))  # some <= 0.5
        _, n, _ = _check_components(mask, (shape, density))
        print(f"COMPONENTS_FRAMES {shape} density {density}: n = {n}")


@pytest.mark.parametrize("shape", [(3, 16, 64), (2, 33, 76)])
def test_components_frames_on_a_mask_that_does_not_start_on_16_bytes(shape):
    n = shape[0] * shape[1] * shape[2]
    assert n % 4 == 0                                                   # only the base keeps it off the 16 B path
    flat = torch.zeros(n + 1, device=DEV)
    mask = flat[1:].view(shape)
    assert mask.data_ptr() % 16 == 4 and mask.is_contiguous()
    mask.copy_((torch.rand(shape, generator=_gen(n)) < 0.3).float().to(DEV))
    _check_components(mask, ("view", shape))


@pytest.mark.parametrize("shape", [(1, 20, 70), (1, 33, 130), (1, 17, 65)])
def test_one_frame_equals_lp_mask_components(shape):
    mask = (torch.rand(shape, generator=_gen(shape[1])) < 0.3).float()
    labels, n, table = _check_components(mask, ("one frame", shape))
    labels2, n2, table2 = detail.mask_components(mask.to(DEV))
    assert n == n2 and torch.equal(labels[0], labels2)
    assert all(row[:2] == (0, 0) for row in table) and tuple(row[2:] for row in table) == table2


def test_connectivity_in_space_and_time():
    def one(voxels, shape=(4, 40, 140)):
        mask = torch.zeros(shape)
        for f, y, x in voxels:
            mask[f, y, x] = 1.0
        return mask

    # a diagonal step in time is adjacent; two frames apart is not -- at a tile corner (15, 63) -> (16, 64)
    _, n, table = _check_components(one([(1, 15, 63), (2, 16, 64)]), "diagonal in time")
    assert n == 1 and table[0] == (1, 2, 15, 16, 63, 64, 2)
    _, n, table = _check_components(one([(0, 15, 63), (2, 16, 64)]), "two frames apart")
    assert n == 2 and table == ((0, 0, 15, 15, 63, 63, 1), (2, 2, 16, 16, 64, 64, 1))
    # the frame below has (f - 1, y, x) unset and two set neighbours that are not adjacent to each other: both must be united
    _, n, _ = _check_components(one([(0, 5, 4), (0, 5, 6), (1, 5, 5)]), "bridge")
    assert n == 1

    # two blobs apart in frame 0 that both touch one blob of frame 1: one component, labelled from frame 0's first voxel
    mask = torch.zeros(3, 40, 140)
    mask[0, 4:10, 10:30] = 1.0
    mask[0, 20:26, 90:110] = 1.0
    mask[1, 9:21, 29:91] = 1.0                                     # touches the first at (9, 29), the second at (20, 90)
    labels, n, table = _check_components(mask, "merge through time")
    assert n == 1 and int(labels[0, 4, 10]) == 1 and table[0] == (0, 1, 4, 25, 10, 109, 2 * 6 * 20 + 12 * 62)

    # a blob that jumps by more than its width per frame splits per frame
    mask = torch.zeros(3, 40, 140)
    for f in range(3):
        mask[f, 10:14, 10 + 6 * f:14 + 6 * f] = 1.0                # 4 wide, 6 a frame: a gap of 2
    assert _check_components(mask, "jump")[1] == 3
    mask = torch.zeros(3, 40, 140)
    for f in range(3):
        mask[f, 10:14, 10 + 4 * f:14 + 4 * f] = 1.0                # its own width a frame: column 13 meets column 14 in time
    assert _check_components(mask, "step")[1] == 1

    # a staircase through time and across tile edges in x and y: one voxel a frame, one step down and right
    F = 40
    stairs = torch.zeros(F, 40, 140)
    for f in range(F):
        stairs[f, f, 40 + f] = 1.0                                  # passes (16, 56), (24, 64) ...: both tile edges
    _, n, table = _check_components(stairs, "staircase")
    assert n == 1 and table[0] == (0, F - 1, 0, F - 1, 40, 40 + F - 1, F)


@pytest.mark.parametrize("shape", [(3, 20, 70), (2, 1, 1), (5, 16, 64)])
def test_components_frames_full_empty_and_the_threshold(shape):
    F, H, W = shape
    _, n, table = _check_components(torch.ones(shape), "full")
    assert n == 1 and table[0] == (0, F - 1, 0, H - 1, 0, W - 1, F * H * W)
    assert _check_components(torch.zeros(shape), "empty")[1:] == (0, ())
    assert _check_components(torch.full(shape, 0.5), "exactly 0.5")[1] == 0              # a strict >
    mask = torch.full(shape, 0.5)
    mask[F - 1, H - 1, W - 1] = 0.5 + 2.0 ** -20
    _, n, table = _check_components(mask, "one above")
    assert n == 1 and table[0] == (F - 1, F - 1, H - 1, H - 1, W - 1, W - 1, 1)


def test_components_frames_past_the_cap_keep_labels_and_count_exact_and_the_table_inside_its_bounds():
    F, H, W = 3, 66, 130
    mask = torch.zeros(F, H, W)
    mask[0::2, 0::2, 0::2] = 1.0                                    # isolated voxels in space and time: 2 * 33 * 65 components
    want_labels, want_n, want_table = subjects_ref.label_frames_ref(mask.numpy() > 0.5)
    assert want_n == 2 * 33 * 65 > CAP
    labels, n, table = _check_components(mask, "past the cap")
    assert n == want_n and len(table) == CAP
    # the raw entry with guard words behind the table: rows past the cap are not written anywhere
    m = mask.to(DEV)
    out = torch.empty((F, H, W), dtype=torch.int32, device=DEV)
    guarded = torch.full((1 + 7 * CAP + 7 * 64,), -7, dtype=torch.int32, device=DEV)
    ws_bytes = _cabi.lp_components_frames_ws_bytes(F, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=DEV)
    assert _cabi.load().lp_mask_components_frames(m.data_ptr(), F, H, W, out.data_ptr(), guarded.data_ptr(), ws.data_ptr(),
                                                  ws_bytes, raw_stream(DEV)) == _cabi.LP_OK
    host = guarded.cpu().numpy()
    assert host[0] == want_n and np.array_equal(host[1:1 + 7 * CAP].reshape(-1, 7), want_table[:CAP])
    assert bool((host[1 + 7 * CAP:] == -7).all()) and np.array_equal(out.cpu().numpy(), want_labels)
    members = detail_subjects.group_subjects((n, table), 64, 4)
    assert members == (tuple(range(1, n + 1)),)
    assert detail_subjects.subject_boxes(labels, members) == (detail.mask_bbox_frames(m),)
    # through the node: one subject, the plan and the crops are the track form's
    image = torch.rand(F, H, W, 3, generator=_gen(9))
    cimg, cmask, st, count = detail_subject_nodes.LanPaint_DetailerCropSubjects().crop(image, mask, 1.0, 0, 0, 8, "bilinear", 1, 64, 4)
    t = detail.plan_track(detail.mask_bbox_frames(m), H, W, 1.0, 0, 8, 0, 1)
    sub = st["subjects"]
    assert count == 1 and sub.members == members and (sub.h, sub.w, sub.oh, sub.ow, sub.origins) == (t.h, t.w, t.oh, t.ow, t.origins)
    old_img, old_mask = detail.crop_track(image.to(DEV), m, t, "bilinear")
    assert np.array_equal(_bits(cimg), _bits(old_img)) and np.array_equal(_bits(cmask), _bits(old_mask))


# ---- lp_subject_boxes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,density", [((4, 33, 130), 0.05), ((3, 17, 65), 0.3), ((2, 300, 70), 0.45)])
def test_subject_boxes_equal_numpy(shape, density):
    S = (torch.rand(shape, generator=_gen(shape[1])) < density).numpy()
    S[1] = False                                                    # a frame nobody is in
    want_labels, n, _ = subjects_ref.label_frames_ref(S)
    assert n >= 8
    labels = torch.from_numpy(want_labels).to(DEV)
    # subject s owns the labels l with l % 5 == s + 1 below two thirds of n; the rest are nobody's, some past the owner table
    members = tuple(tuple(l for l in range(1, 2 * n // 3) if l % 5 == s + 1) for s in range(3))
    boxes = detail_subjects.subject_boxes(labels, members)
    assert np.array_equal(np.array(boxes, np.int64), subjects_ref.subject_boxes_ref(want_labels, members))
    assert all(boxes[s][1] == (shape[1], -1, shape[2], -1) for s in range(3))
    one = detail_subjects.subject_boxes(labels, (tuple(range(1, n + 1)),))                # every label: the mask's own boxes
    assert one == (detail.mask_bbox_frames(torch.from_numpy(S).float().to(DEV)),)


# ---- the scene: two boxes that cross, a small blob that appears late ---------------------------------------------------------------
F0, H0, W0 = 6, 48, 96


def _crossing(seed=7, soft=True):
    """6 frames of 48 x 96: an 8 x 10 box at rows 4..11 moving right 10 a frame, a 10 x 10 box at rows 30..39 moving left 10 a
    frame, a 4 x 4 blob at rows 20..23 in the last two frames.  Components 1, 2, 3 of volumes 480, 600, 32."""
    S = torch.zeros(F0, H0, W0, dtype=torch.bool)
    for f in range(F0):
        S[f, 4:12, 5 + 10 * f:15 + 10 * f] = True
        S[f, 30:40, 80 - 10 * f:90 - 10 * f] = True
    S[4:, 20:24, 44:48] = True
    if not soft:
        return S.float()
    noise = torch.rand(S.shape, generator=_gen(seed))
    return torch.where(S, 0.55 + 0.45 * noise, 0.3 * noise * (noise > 0.8))              # soft: nobody's values at or below 0.5


@pytest.fixture(scope="module")
def crossing():
    """The scene labelled once: (mask CPU, labels on the device, labels as numpy, n, table)."""
    mask = _crossing()
    labels, n, table = _check_components(mask, "crossing")
    assert n == 3 and [row[6] for row in table] == [480, 600, 32]
    assert table[0][:2] == (0, 5) and table[2][:2] == (4, 5)
    return mask, labels, labels.cpu().numpy(), n, table


def _plan(crossing, target, padding=12, max_subjects=4, min_area=1, smooth=3):
    mask, labels, _, n, table = crossing
    members = detail_subjects.group_subjects((n, table), min_area, max_subjects)
    boxes = detail_subjects.subject_boxes(labels, members)
    return detail_subjects.plan_subjects(members, boxes, H0, W0, 1.0, padding, 8, target, smooth)


@pytest.mark.parametrize("target", [0, 64])
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("c", [1, 3])
def test_crop_subjects_is_crop_resample_per_subject_and_frame_bit_for_bit(crossing, c, filter, target):
    mask, labels, ref_labels, _, _ = crossing
    sub = _plan(crossing, target)
    assert sub.subjects == 3 and sub.frames == F0 and sub.resampled == (target > 0) and sub.members == ((1,), (2,), (3,))
    image = torch.rand(F0, H0, W0, c, generator=_gen(11 + c))
    cimg, cmask = detail_subjects.crop_subjects(image.to(DEV), mask.to(DEV), sub, labels, filter)
    assert tuple(cimg.shape) == (3 * F0, sub.oh, sub.ow, c) and tuple(cmask.shape) == (3 * F0, sub.oh, sub.ow)
    foreign_seen = 0
    for s in range(3):
        ms = subjects_ref.subject_mask(mask, ref_labels, sub.members[s])
        for f in range(F0):
            r = sub.window(s, f)
            foreign = (ref_labels[f, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w] != 0) & \
                ~np.isin(ref_labels[f, r.y0:r.y0 + r.h, r.x0:r.x0 + r.w], sub.members[s])
            foreign_seen += int(foreign.sum())
            wimg, wmask = detail.crop_resample(image[f:f + 1].to(DEV), ms[f:f + 1].to(DEV), r, filter)
            assert np.array_equal(_bits(cimg[s * F0 + f]), _bits(wimg[0])), (s, f)
            assert np.array_equal(_bits(cmask[s * F0 + f]), _bits(wmask[0])), (s, f)
            if target == 0:
                assert bool((cmask[s * F0 + f].cpu()[torch.from_numpy(foreign)] == 0).all())
    assert foreign_seen > 0                                         # a foreign subject lies inside some window
    plain, _ = detail_subjects.crop_subjects(image.to(DEV), None, sub, None, filter)
    assert np.array_equal(_bits(plain), _bits(cimg))
    _, asis = detail_subjects.crop_subjects(image.to(DEV), mask.to(DEV), sub, None, filter)       # no labels: the mask as it is
    want = detail.crop_resample(image[2:3].to(DEV), mask[2:3].to(DEV), sub.window(1, 2), filter)[1]
    assert np.array_equal(_bits(asis[1 * F0 + 2]), _bits(want[0]))


def _compose_parent(original, det, mask, ref_labels, sub, k, filter):
    out = original.to(DEV).clone()
    for s in range(sub.subjects):
        ms = subjects_ref.subject_mask(mask, ref_labels, sub.members[s]).to(DEV)
        for f in range(sub.frames):
            i = s * sub.frames + f
            out[f:f + 1] = detail.stitch(out[f:f + 1].contiguous(), det[i:i + 1].to(DEV), ms[f:f + 1], sub.window(s, f), k, filter)
    return out


def _outside_windows_untouched(out, original, sub):
    outside = torch.from_numpy(subjects_ref.cover_count(sub) == 0)
    return bool(outside.any()) and np.array_equal(_bits(out[outside]), _bits(original[outside]))


@pytest.mark.parametrize("filter,target", [("bilinear", 0), ("bicubic", 64)])
@pytest.mark.parametrize("k", [1, 9, 17])                           # 17 > 15: the 8 x 32 tile
@pytest.mark.parametrize("c", [3, 1])
def test_stitch_subjects_is_the_composition_of_stitch_and_meets_the_torch_restatement(crossing, c, k, filter, target):
    mask, labels, ref_labels, _, _ = crossing
    sub = _plan(crossing, target, padding=6 if target == 0 else 12)
    cover = int(subjects_ref.cover_count(sub).max())
    assert sub.subjects == 3 and sub.resampled == (target > 0) and cover >= 2      # windows of different subjects overlap
    image = torch.rand(F0, H0, W0, c, generator=_gen(40 + k))
    det = torch.rand(3 * F0, sub.oh, sub.ow, c, generator=_gen(50 + k))
    out = detail_subjects.stitch_subjects(image.to(DEV), det.to(DEV), mask.to(DEV), sub, labels, k, filter)
    assert out.is_cuda and out.dtype == torch.float32
    want = _compose_parent(image, det, mask, ref_labels, sub, k, filter)
    assert np.array_equal(_bits(out), _bits(want))                  # bit for bit, every element
    out = out.cpu()
    assert _outside_windows_untouched(out, image, sub)
    ref = subjects_ref.stitch_subjects_ref(image, det, mask, sub, ref_labels, k, filter)
    bnd = detail_ref.bound((sub.oh, sub.ow), (sub.h, sub.w), filter, float(det.abs().max()))
    err = float((out - ref).abs().max())
    print(f"STITCH_SUBJECTS k={k} {filter} target={target} cover={cover}: max err {err:.3g}, atol {cover * (3e-6 + bnd):.3g}")
    assert err <= cover * (3e-6 + bnd)                              # the tolerance of stitch_regions' restatement check


def test_stitch_subjects_without_labels_uses_the_mask_as_it_is(crossing):
    mask, _, ref_labels, _, _ = crossing
    sub = _plan(crossing, 0)
    image = torch.rand(F0, H0, W0, 3, generator=_gen(3))
    det = torch.rand(3 * F0, sub.oh, sub.ow, 3, generator=_gen(4))
    out = detail_subjects.stitch_subjects(image.to(DEV), det.to(DEV), mask.to(DEV), sub, None, 9)
    everyone = dataclasses.replace(sub, members=tuple((1, 2, 3) for _ in range(3)))      # nobody is foreign to anybody
    want = _compose_parent(image, det, mask, ref_labels, everyone, 9, "bilinear")
    assert np.array_equal(_bits(out), _bits(want))


def test_wrappers_check_the_subjects_against_the_batch(crossing):
    mask, labels, _, _, _ = crossing
    sub = _plan(crossing, 0)
    image = torch.rand(F0, H0, W0, 3, generator=_gen(5)).to(DEV)
    with pytest.raises(ValueError, match="region nodes"):
        detail_subjects.crop_subjects(image, mask[:1].to(DEV), sub, labels)
    with pytest.raises(ValueError):
        detail_subjects.crop_subjects(image[:4], mask[:4].to(DEV), sub, labels[:4].contiguous())
    with pytest.raises(ValueError):
        detail_subjects.crop_subjects(image, mask.to(DEV), sub, labels[0])                 # a label plane, not a volume
    with pytest.raises(ValueError):
        detail_subjects.stitch_subjects(image, image[:, :sub.oh, :sub.ow], mask.to(DEV), sub, labels, 9)   # F crops, not S * F
    with pytest.raises(ValueError):
        detail_subjects.stitch_subjects(image, torch.zeros(3 * F0, sub.oh, sub.ow, 3, device=DEV), mask.to(DEV), sub, labels, 4)


# ---- nodes ---------------------------------------------------------------------------------------------------------------------------
def _disc_clip(frames, H, W, radius, x_from, x_to, cy):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(frames, H, W)
    for f in range(frames):
        cx = x_from + (x_to - x_from) * f // max(frames - 1, 1)
        mask[f] = (((yy - cy - (f % 3)) ** 2 + (xx - cx) ** 2) < radius * radius).float()
    return mask


@pytest.mark.parametrize("filter,target", [("bicubic", 0), ("bilinear", 96)])
def test_subject_nodes_with_one_moving_blob_equal_the_track_nodes_bit_for_bit(filter, target):
    frames, H, W = 8, 64, 160
    image = torch.rand(frames, H, W, 3, generator=_gen(31))
    mask = _disc_clip(frames, H, W, 9, 20, 132, 30)                 # 16 a frame, 17 wide: one component
    old_img, old_mask, old_st = detail_track_nodes.LanPaint_DetailerCropTrack().crop(image, mask, 1.25, 4, target, 8, filter, 3)
    cimg, cmask, st, count = detail_subject_nodes.LanPaint_DetailerCropSubjects().crop(image, mask, 1.25, 4, target, 8, filter,
                                                                                       3, 1, 4)
    sub, track = st["subjects"], old_st["track"]
    assert count == 1 and sub.members == ((1,),) and sub.origins == track.origins and len(set(sub.origins)) > 4
    assert (sub.h, sub.w, sub.oh, sub.ow) == (track.h, track.w, track.oh, track.ow)
    assert cimg.device.type == "cpu" and cmask.device.type == "cpu"
    assert np.array_equal(_bits(cimg), _bits(old_img)) and np.array_equal(_bits(cmask), _bits(old_mask))
    inpainted = (cimg * 0.5 + 0.25).contiguous()
    old_out, = detail_track_nodes.LanPaint_DetailerStitchTrack().stitch(old_st, inpainted, 9)
    out, = detail_subject_nodes.LanPaint_DetailerStitchSubjects().stitch(copy.deepcopy(st), inpainted, 9)
    assert out.device.type == "cpu" and np.array_equal(_bits(out), _bits(old_out))
    with pytest.raises(ValueError, match="region nodes"):
        detail_subject_nodes.LanPaint_DetailerCropSubjects().crop(image, mask[:1], 1.25, 4, target, 8, filter, 3, 1, 4)


@pytest.mark.parametrize("k", [1, 9])
def test_subject_nodes_on_two_blobs_that_cross(k):
    mask = _crossing(soft=False)
    image = torch.rand(F0, H0, W0, 3, generator=_gen(21)) * 0.5 + 0.25
    crop, stitch = detail_subject_nodes.LanPaint_DetailerCropSubjects(), detail_subject_nodes.LanPaint_DetailerStitchSubjects()
    cimg, cmask, st, count = crop.crop(image, mask, 1.0, 4, 0, 8, "bicubic", 1, 1, 4)
    sub = st["subjects"]
    assert count == 3 and sub.members == ((1,), (2,), (3,)) and tuple(cimg.shape) == (3 * F0, sub.h, sub.w, 3)
    ref_labels = st["labels"].cpu().numpy()
    for s in range(3):
        ms = subjects_ref.subject_mask(mask, ref_labels, sub.members[s])
        for f in range(F0):
            y0, x0 = sub.origins[s * F0 + f]
            assert torch.equal(cimg[s * F0 + f], image[f, y0:y0 + sub.h, x0:x0 + sub.w, :])
            assert torch.equal(cmask[s * F0 + f], ms[f, y0:y0 + sub.h, x0:x0 + sub.w])
            assert float(cmask[s * F0 + f].sum()) == float(ms[f].sum())                # a subject's mask lies inside its window
    assert crop.crop(image, mask, 1.0, 4, 0, 8, "bicubic", 1, 17, 4)[3] == 2            # the blob's mean area is 16: dropped
    assert crop.crop(image, mask, 1.0, 4, 0, 8, "bicubic", 1, 1, 2)[3] == 2             # merged instead
    # an identity "inpaint" round-trips
    out, = stitch.stitch(copy.deepcopy(st), cimg, k)
    assert out.device.type == "cpu" and _outside_windows_untouched(out, image, sub)
    # o * (1 - m) + o * m once per covering window: the bound of the existing round trips, a few roundings of o, per cover
    cover = int(subjects_ref.cover_count(sub).max())
    assert bool(((out - image).abs() <= cover * 5 * 2.0 ** -24 * image.abs()).all())
    # halved brightness for subject 0 alone leaves subject 1's mask area untouched, and changes subject 0's
    inpainted = cimg.clone()
    inpainted[:F0] *= 0.5
    half, = stitch.stitch(copy.deepcopy(st), inpainted, k)
    own = torch.from_numpy(ref_labels == 1)
    other = torch.from_numpy(ref_labels == 2)
    assert np.array_equal(_bits(half[other]), _bits(out[other]))
    assert bool((half[own] < 0.75 * image[own]).all())
    # the colour match node runs on the stack with clip_frames = F
    matched, = detail_color_nodes.LanPaint_DetailerColorMatch().match(inpainted, cimg, cmask, "mean_std", 1.0, 2, 3, F0)
    assert tuple(matched.shape) == tuple(cimg.shape) and bool(torch.isfinite(matched).all())


# ---- one moderate size ---------------------------------------------------------------------------------------------------------------
def test_three_moving_discs_at_a_moderate_size():
    frames, H, W = 12, 270, 480
    mask = torch.maximum(torch.maximum(_disc_clip(frames, H, W, 20, 60, 420, 70), _disc_clip(frames, H, W, 20, 420, 60, 180)),
                         _disc_clip(frames, H, W, 10, 200, 280, 125))
    mask[:8, 100:150] = 0.0                                         # the small disc appears late
    labels, n, table = _check_components(mask, "three discs")
    assert n == 3 and [row[:2] for row in table] == [(0, 11), (0, 11), (8, 11)]
    members = detail_subjects.group_subjects((n, table), 64, 4)
    boxes = detail_subjects.subject_boxes(labels, members)
    ref_labels = labels.cpu().numpy()
    assert np.array_equal(np.array(boxes, np.int64), subjects_ref.subject_boxes_ref(ref_labels, members))
    sub = detail_subjects.plan_subjects(members, boxes, H, W, 1.25, 8, 8, 96, 3)
    assert sub.subjects == 3 and sub.w < W // 3 and sub.resampled
    image = torch.rand(frames, H, W, 3, generator=_gen(61))
    cimg, cmask = detail_subjects.crop_subjects(image.to(DEV), mask.to(DEV), sub, labels, "bicubic")
    det = (cimg * 0.5 + 0.25).contiguous()
    out = detail_subjects.stitch_subjects(image.to(DEV), det, mask.to(DEV), sub, labels, 9, "bicubic")
    want = _compose_parent(image, det.cpu(), mask, ref_labels, sub, 9, "bicubic")
    assert np.array_equal(_bits(out), _bits(want))
    assert _outside_windows_untouched(out.cpu(), image, sub)
