"""The Detailer that follows a moving mask, on the MI355X (lanpaint_amd.detail, csrc/detail_kernel.hip): lp_mask_bbox_frames
against a numpy restatement and against lp_mask_bbox plane by plane, lp_detail_resample_track and lp_detail_stitch_track bit for
bit against the single-window entries called once per frame, the untouched outside of every frame's window, and the two nodes.
Every comparison covers every element."""
import copy

import numpy as np
import pytest
import torch

from lanpaint_amd import blend, detail, detail_nodes, detail_track_nodes
from tests.compare import _tensor_bits as _bits
from tests.device import DEV, _gen
from tests.image_checks import _window_mask
from tests.image_inputs import _boxes_ref

pytestmark = pytest.mark.gpu


# ---- lp_mask_bbox_frames -----------------------------------------------------------------------------------------------------------
def _check_boxes(mask, what):
    """mask: CPU tensor, or a HIP tensor to be used as it is (its alignment matters)."""
    dev_mask = mask if mask.is_cuda else mask.to(DEV)
    got = detail.mask_bbox_frames(dev_mask)
    want = _boxes_ref(mask)
    assert got == want, (what, [(p, g, w) for p, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    planes = dev_mask if dev_mask.ndim == 3 else dev_mask.unsqueeze(0)
    for p in range(planes.shape[0]):                                     # row p is lp_mask_bbox of plane p alone
        assert detail.mask_bbox(planes[p]) == got[p], (what, p)
    rows = np.array(got)
    union = (int(rows[:, 0].min()), int(rows[:, 1].max()), int(rows[:, 2].min()), int(rows[:, 3].max()))
    assert detail.mask_bbox(dev_mask) == union, what                     # and the rows reduce to the box over every plane
    return got


def _soft_sparse(shape, density, seed):
    g = _gen(seed)
    mask = (torch.rand(shape, generator=g) < density).float() * torch.rand(shape, generator=g)    # soft values, some <= 0.5
    if mask.ndim == 3 and shape[0] > 2:
        mask[2::4] = mask[2::4].clamp(max=0.5)                           # empty planes: soft values at or below 0.5 only
    return mask


@pytest.mark.parametrize("shape", [(1, 16, 64), (7, 33, 77), (3, 257, 1003), (130, 70)])
def test_bbox_frames_equals_numpy_and_mask_bbox_per_plane(shape):
    for density in (0.0005, 0.01, 0.3):
        mask = _soft_sparse(shape, density, shape[-1])
        got = _check_boxes(mask, (shape, density))
        if len(shape) == 3 and shape[0] > 2:
            assert got[2] == (shape[1], -1, shape[2], -1)
    view = _soft_sparse((7, 33, 77), 0.05, 5).to(DEV)[:, :, 3:]          # a strided view: made contiguous by the wrapper
    assert not view.is_contiguous()
    _check_boxes(view, "view")


def test_bbox_frames_at_video_size():
    planes, H, W = 81, 720, 1280
    mask = _soft_sparse((planes, H, W), 0.0002, 9)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for f in range(planes):
        if f % 4 != 2:
            blob = ((yy - (300 + f)) ** 2 + (xx - (200 + 10 * f)) ** 2) < 60 * 60
            mask[f][blob] = 0.75
    got = _check_boxes(mask, "video")
    assert len(got) == 81 and got[2] == (H, -1, W, -1) and got[80][1] - got[80][0] >= 118


@pytest.mark.parametrize("H,W", [(64, 256), (37, 101), (1, 1), (500, 1300)])
def test_bbox_frames_single_pixels_at_each_corner_the_threshold_and_empty_planes(H, W):
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)]
    mask = torch.zeros(len(corners) + 3, H, W)
    for p, (y, x) in enumerate(corners):
        mask[p, y, x] = 1.0
    mask[5] = 0.5                                                        # 0.5 itself is not set
    mask[6] = 0.5
    mask[6, H // 3, W // 4] = float(np.nextafter(np.float32(0.5), np.float32(0)))
    mask[6, H // 2, W // 2] = float(np.nextafter(np.float32(0.5), np.float32(1)))
    got = _check_boxes(mask, "corners")
    assert got[:5] == tuple((y, y, x, x) for y, x in corners)
    assert got[5] == (H, -1, W, -1) and got[6] == (H // 2, H // 2, W // 2, W // 2) and got[7] == (H, -1, W, -1)
    with pytest.raises(ValueError, match="empty"):
        detail.plan_track(detail.mask_bbox_frames(torch.zeros(3, H, W, device=DEV)), H, W)


@pytest.mark.parametrize("shape", [(3, 32, 128), (2, 33, 76), (3, 50, 66)])
def test_bbox_frames_on_a_mask_that_does_not_start_on_16_bytes(shape):
    """The 16-bytes-per-lane path needs W % 4 == 0 and an aligned base; everything else takes the scalar path."""
    mask = _soft_sparse(shape, 0.02, shape[1])
    n_el = mask.numel()
    for offset in (0, 1, 2):
        buf = torch.zeros(n_el + 4, device=DEV)
        view = buf[offset:offset + n_el].view(shape)
        view.copy_(mask)
        assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
        assert detail.mask_bbox_frames(view) == _boxes_ref(mask), (shape, offset)


# ---- scenes for crop and stitch ------------------------------------------------------------------------------------------------------
H0, W0, WIN = 90, 131, (40, 56)                                          # W * C is a multiple of 4 only for C = 4
# one window flush with each corner of the image, each border, and one inside
ORIGINS = ((0, 0), (0, W0 - WIN[1]), (H0 - WIN[0], 0), (H0 - WIN[0], W0 - WIN[1]), (23, 31), (0, 40), (50, 17), (11, 75))
SIZES = {"copy": WIN, "up": (96, 136), "down": (24, 32)}


def _track(size, origins=ORIGINS):
    return detail.Track(H0, W0, WIN[0], WIN[1], SIZES[size][0], SIZES[size][1], tuple(origins))


def _moving_mask(track, planes, seed):
    """A soft mask whose set rectangle sits inside each frame's window (touching its edge in some frames), soft background."""
    mask = torch.zeros(planes, track.H, track.W)
    for p in range(planes):
        y0, x0 = track.origins[p]
        mask[p, y0 + 6 - 6 * (p % 2):y0 + 30, x0 + 9:x0 + track.w - 8 * (p % 3)] = 1.0
    noise = torch.rand(mask.shape, generator=_gen(seed))
    return torch.where(mask > 0, 0.55 + 0.45 * noise, 0.3 * noise * (noise > 0.8))


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("c", [1, 3, 4])
def test_crop_track_is_crop_resample_per_frame_bit_for_bit(c, filter, size):
    track = _track(size)
    b = len(track)
    image = torch.randn(b, H0, W0, c, generator=_gen(10 * c + len(size)))
    mask = _moving_mask(track, b, 3 + c)
    before_img, before_mask = image.clone(), mask.clone()
    img_d, mask_d = image.to(DEV), mask.to(DEV)
    cimg, cmask = detail.crop_track(img_d, mask_d, track, filter)
    assert cimg.is_cuda and cimg.dtype == torch.float32 and tuple(cimg.shape) == (b, track.oh, track.ow, c)
    assert tuple(cmask.shape) == (b, track.oh, track.ow) and track.resampled == (size != "copy")
    for f in range(b):
        want_img, want_mask = detail.crop_resample(img_d[f:f + 1], mask_d[f:f + 1], track.region(f), filter)
        assert np.array_equal(_bits(cimg[f:f + 1]), _bits(want_img)), (f, "image")
        assert np.array_equal(_bits(cmask[f:f + 1]), _bits(want_mask)), (f, "mask")
    only_img, none = detail.crop_track(img_d, None, track, filter)
    assert none is None and np.array_equal(_bits(only_img), _bits(cimg))
    assert np.array_equal(_bits(img_d), _bits(before_img)) and np.array_equal(_bits(mask_d), _bits(before_mask))   # inputs untouched


@pytest.mark.parametrize("size", ["copy", "up"])
def test_crop_track_with_a_one_plane_mask(size):
    moving = _track(size)
    b = len(moving)
    image = torch.rand(b, H0, W0, 3, generator=_gen(2)).to(DEV)
    mask = _moving_mask(moving, 1, 4).to(DEV)
    _, cmask = detail.crop_track(image, mask, moving, "bicubic")         # a track that moves: the plane is cut once per frame
    assert tuple(cmask.shape) == (b, moving.oh, moving.ow)
    for f in range(b):
        _, want = detail.crop_resample(image[f:f + 1], mask, moving.region(f), "bicubic")
        assert np.array_equal(_bits(cmask[f:f + 1]), _bits(want)), f
    still = _track(size, (ORIGINS[4],) * b)                              # a track that stands still: one plane in, one plane out
    cimg, cmask = detail.crop_track(image, mask, still, "bicubic")
    want_img, want_mask = detail.crop_resample(image, mask, still.region(0), "bicubic")
    assert tuple(cmask.shape) == (1, still.oh, still.ow)
    assert np.array_equal(_bits(cimg), _bits(want_img)) and np.array_equal(_bits(cmask), _bits(want_mask))
    _, cmask2 = detail.crop_track(image, mask[0], still, "bicubic")      # a 2-D mask
    assert np.array_equal(_bits(cmask2), _bits(want_mask))


@pytest.mark.parametrize("size", ["copy", "up", "down"])
@pytest.mark.parametrize("filter", detail.FILTERS)
@pytest.mark.parametrize("k", [1, 9, 51])
@pytest.mark.parametrize("c,mask_per_frame", [(3, True), (4, False), (1, True)])
def test_stitch_track_is_stitch_per_frame_bit_for_bit_and_leaves_the_outside_alone(c, mask_per_frame, k, filter, size):
    track = _track(size)
    b = len(track)
    original = torch.rand(b, H0, W0, c, generator=_gen(40 + k))
    mask = _moving_mask(track, b if mask_per_frame else 1, 50 + k)
    if not mask_per_frame:
        mask[0, 20:70, 30:100] = 0.9                                     # one plane that reaches into every frame's window
    det = torch.rand(b, track.oh, track.ow, c, generator=_gen(60 + k))
    orig_d, det_d, mask_d = original.to(DEV), det.to(DEV), mask.to(DEV)
    out = detail.stitch_track(orig_d, det_d, mask_d, track, k, filter)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(original.shape)
    changed = 0
    for f in range(b):
        mf = mask_d[f:f + 1] if mask_per_frame else mask_d
        want = detail.stitch(orig_d[f:f + 1], det_d[f:f + 1], mf, track.region(f), k, filter)
        assert np.array_equal(_bits(out[f:f + 1]), _bits(want)), f
        changed += int((want.cpu() != original[f:f + 1]).sum())
    assert changed > 0
    out = out.cpu()
    outside = ~_window_mask(track)
    assert bool(outside.flatten(1).any(dim=1).all()) and np.array_equal(_bits(out[outside]), _bits(original[outside]))
    assert np.array_equal(_bits(orig_d), _bits(original)) and np.array_equal(_bits(mask_d), _bits(mask))           # inputs untouched
    assert np.array_equal(_bits(det_d), _bits(det))


@pytest.mark.parametrize("size", ["copy", "up"])
@pytest.mark.parametrize("filter", detail.FILTERS)
def test_constant_track_equals_the_existing_detailer_bit_for_bit(filter, size):
    b = 4
    track = _track(size, (ORIGINS[4],) * b)
    region = track.region(0)
    for mask_b in (1, b):
        image = torch.rand(b, H0, W0, 3, generator=_gen(7)).to(DEV)
        mask = _moving_mask(track, mask_b, 8).to(DEV)
        cimg, cmask = detail.crop_track(image, mask, track, filter)
        want_img, want_mask = detail.crop_resample(image, mask, region, filter)
        assert np.array_equal(_bits(cimg), _bits(want_img)) and np.array_equal(_bits(cmask), _bits(want_mask))
        det = (cimg * 0.5 + 0.25).contiguous()
        for k in (1, 9, 51):
            out = detail.stitch_track(image, det, mask, track, k, filter)
            assert np.array_equal(_bits(out), _bits(detail.stitch(image, det, mask, region, k, filter))), (mask_b, k)


def test_wrappers_check_the_track_against_the_batch():
    track = _track("copy")
    image = torch.rand(len(track), H0, W0, 3, generator=_gen(1)).to(DEV)
    mask = _moving_mask(track, len(track), 2).to(DEV)
    with pytest.raises(ValueError, match="frames"):
        detail.crop_track(image[:3], mask[:3], track)
    with pytest.raises(ValueError, match="leaves"):
        detail.crop_track(image, mask, _track("copy", ORIGINS[:-1] + ((H0 - WIN[0] + 1, 0),)))
    with pytest.raises(ValueError, match="mask shape"):
        detail.crop_track(image, mask[:3], track)
    with pytest.raises(ValueError, match="detail_img"):
        detail.stitch_track(image, image, mask, track, 9)


# ---- nodes ---------------------------------------------------------------------------------------------------------------------------
def _blob_clip(frames, H, W, radius, x_from, x_to, hole=()):
    """A disc that moves from x_from to x_to at constant speed, one mask per frame; the frames in `hole` are empty."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = torch.zeros(frames, H, W)
    for f in range(frames):
        if f in hole:
            continue
        cx = x_from + (x_to - x_from) * f // max(frames - 1, 1)
        cy = H // 2 + (f % 5) - 2
        mask[f] = (((yy - cy) ** 2 + (xx - cx) ** 2) < radius * radius).float()
    return mask


def _smoothed(mask, image, k):
    """m as the kernels compute it (lp_mask_blend's smooth_out runs the same tile passes), [B, H, W] on the CPU."""
    _, m = blend._launch(mask.to(DEV), image.to(DEV), image.to(DEV), k, want_smooth=True)
    return m.cpu()


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("smooth", [1, 9])
def test_track_nodes_round_trip_identity_inpaint_without_resample(smooth, k):
    frames, H, W = 12, 96, 260
    image = torch.rand(frames, H, W, 3, generator=_gen(21))
    mask = _blob_clip(frames, H, W, 14, 30, 225, hole=(0, 5, 6, 11))
    cimg, cmask, st = detail_track_nodes.LanPaint_DetailerCropTrack().crop(image, mask, 1.5, 8, 0, 8, "bicubic", smooth)
    track = st["track"]
    assert cimg.device.type == "cpu" and cmask.device.type == "cpu" and not track.resampled and len(track) == frames
    assert track == detail.plan_track(detail.mask_bbox_frames(mask.to(DEV)), H, W, 1.5, 8, 8, 0, smooth)
    assert len(set(track.origins)) > 4 and track.w < W // 2              # the window moves and is far smaller than the union box
    for f, (y0, x0) in enumerate(track.origins):
        assert torch.equal(cimg[f], image[f, y0:y0 + track.h, x0:x0 + track.w, :])
        assert torch.equal(cmask[f], mask[f, y0:y0 + track.h, x0:x0 + track.w])
        assert float(cmask[f].sum()) == float(mask[f].sum())             # every frame's mask lies inside its window
    out, = detail_track_nodes.LanPaint_DetailerStitchTrack().stitch(copy.deepcopy(st), cimg, k)
    assert out.device.type == "cpu"
    outside = ~_window_mask(track)
    assert np.array_equal(_bits(out[outside]), _bits(image[outside]))
    m = _smoothed(mask, image, k).unsqueeze(-1).expand_as(image)
    exact = (m == 0) | (m == 1)
    assert torch.equal(out[exact], image[exact])
    # o * (1 - m) + o * m: the bound of the existing stitch round trip (tests/test_gpu_detail.py), a few roundings of o
    assert bool(((out - image).abs() <= 5 * 2.0 ** -24 * image.abs()).all())
    if k > 1:
        assert bool((~exact).any())


@pytest.mark.parametrize("target", [0, 128])
def test_track_nodes_recolour_appears_only_under_the_smoothed_mask_inside_each_window(target):
    frames, H, W, k = 10, 96, 260, 9
    image = torch.rand(frames, H, W, 3, generator=_gen(31)) * 0.2        # dark, so that the recolour below differs everywhere
    mask = _blob_clip(frames, H, W, 14, 225, 30, hole=(3,))
    cimg, cmask, st = detail_track_nodes.LanPaint_DetailerCropTrack().crop(image, mask, 1.25, 4, target, 8, "bilinear", 9)
    track = st["track"]
    assert track.resampled == (target > 0) and tuple(cimg.shape) == (frames, track.oh, track.ow, 3)
    inpainted = (cimg * 0.5 + 0.6).contiguous()                          # the recolouring "sampler"
    out, = detail_track_nodes.LanPaint_DetailerStitchTrack().stitch(copy.deepcopy(st), inpainted, k)
    want = detail.stitch_track(image.to(DEV), inpainted.to(DEV), mask.to(DEV), track, k, "bilinear")
    assert out.device.type == "cpu" and np.array_equal(_bits(out), _bits(want))
    m = _smoothed(mask, image, k)
    allowed = (m > 0) & _window_mask(track)
    changed = (out != image).any(dim=-1)
    assert not bool((changed & ~allowed).any())
    assert bool((changed == allowed).all())                              # and everywhere it may: 0.6 + is far from < 0.2
    assert not bool(changed[3].any()) and bool(changed[4].any())         # the frame without a mask comes back as it went in


def test_static_mask_through_the_track_nodes_equals_the_existing_nodes():
    frames, H, W = 4, 96, 160
    image = torch.rand(frames, H, W, 3, generator=_gen(41))
    mask = torch.zeros(1, H, W)
    mask[0, 30:61, 50:91] = 1.0
    old_img, old_mask, old_st = detail_nodes.LanPaint_DetailerCrop().crop(image, mask, 1.0, 0, 0, 8, "bicubic")
    cimg, cmask, st = detail_track_nodes.LanPaint_DetailerCropTrack().crop(image, mask, 1.0, 0, 0, 8, "bicubic", 9)
    track, region = st["track"], old_st["region"]
    assert len(track) == frames and len(set(track.origins)) == 1 and (track.h, track.w) == (region.h, region.w)
    same_place = track.origins[0] == (region.y0, region.x0)
    out, = detail_track_nodes.LanPaint_DetailerStitchTrack().stitch(st, (cimg * 0.5).contiguous(), 9)
    want = detail.stitch(image.to(DEV), (cimg * 0.5).contiguous().to(DEV), mask.to(DEV), track.region(0), 9, "bicubic")
    assert np.array_equal(_bits(out), _bits(want)) and tuple(cmask.shape) == (1, track.oh, track.ow)
    if same_place:
        assert np.array_equal(_bits(cimg), _bits(old_img)) and np.array_equal(_bits(cmask), _bits(old_mask))


# ---- one run at video size -------------------------------------------------------------------------------------------------------------
def test_track_at_video_size_frames_0_40_80_equal_the_per_frame_calls():
    frames, H, W = 81, 720, 1280
    mask = _blob_clip(frames, H, W, 60, 200, 1000)
    image = torch.rand(frames, H, W, 3, generator=_gen(51))
    mask_d, image_d = mask.to(DEV), image.to(DEV)
    boxes = detail.mask_bbox_frames(mask_d)
    assert len(boxes) == frames and boxes == _boxes_ref(mask)
    track = detail.plan_track(boxes, H, W, 1.5, 32, 8, 512, 9)
    union = detail.plan_region(detail.mask_bbox(mask_d), H, W, 1.5, 32, 8, 512)
    print(f"TRACK video: window {track.h}x{track.w} -> {track.oh}x{track.ow}; union region {union.h}x{union.w} -> {union.oh}x{union.ow}")
    assert track.resampled and track.w * 3 < union.w and len(set(track.origins)) > 40
    cimg, cmask = detail.crop_track(image_d, mask_d, track, "bicubic")
    det = (cimg * 0.5 + 0.25).contiguous()
    out = detail.stitch_track(image_d, det, mask_d, track, 9, "bicubic")
    for f in (0, 40, 80):
        want_img, want_mask = detail.crop_resample(image_d[f:f + 1], mask_d[f:f + 1], track.region(f), "bicubic")
        assert np.array_equal(_bits(cimg[f:f + 1]), _bits(want_img)) and np.array_equal(_bits(cmask[f:f + 1]), _bits(want_mask)), f
        want = detail.stitch(image_d[f:f + 1], det[f:f + 1], mask_d[f:f + 1], track.region(f), 9, "bicubic")
        assert np.array_equal(_bits(out[f:f + 1]), _bits(want)), f
        assert bool((want != image_d[f:f + 1]).any())
    outside = (~_window_mask(track)).to(DEV)                             # compared on the device: 81 frames are large
    assert bool(outside.any()) and torch.equal(out.view(torch.int32)[outside], image_d.view(torch.int32)[outside])


# ---- the device-side origin clamp, through the C entries ------------------------------------------------------------------------------
# The header promises for every device table that "an origin is clamped so that its window lies inside the image"; the Python
# wrappers refuse such tables, so only a raw call reaches the clamp.  Every tensor a window indexes is the middle of one with a
# guard frame before and after: an origin left unclamped by up to 3 rows still reads and writes allocated memory, and the test
# fails by value.
_CLAMP_H, _CLAMP_W, _CLAMP_WIN = 23, 31, (8, 12)
_CLAMP_ORIGINS = ((-3, -2), (_CLAMP_H - 8 + 3, _CLAMP_W - 12 + 1), (5, 7))
# two subjects on the same three frames, subject-major: subject 0's row is the table above; each side of each axis is left once
_CLAMP_SUBJECT_ORIGINS = _CLAMP_ORIGINS + ((2, -1), (-1, _CLAMP_W - 12 + 3), (_CLAMP_H - 8 + 1, 9))
_GUARD = -7.0


def _clamped(origins):
    h, w = _CLAMP_WIN
    return tuple((min(max(y, 0), _CLAMP_H - h), min(max(x, 0), _CLAMP_W - w)) for y, x in origins)


def _guarded(frames, *rest, seed=None):
    """(whole, middle): `frames` frames between two guard frames; random in the middle with `seed`, the guard value without."""
    whole = torch.full((frames + 2, *rest), _GUARD)
    if seed is not None:
        whole[1:-1] = torch.rand(frames, *rest, generator=_gen(seed))
    whole = whole.to(DEV)
    return whole, whole[1:-1]


def _axis_tables(n_in, n_out):
    bounds, weights = detail.aa_coeffs(n_in, n_out, "bilinear")
    return torch.from_numpy(bounds.copy()).to(DEV), torch.from_numpy(weights.astype(np.float32)).to(DEV)


def _raw(entry, desc):
    import ctypes
    from lanpaint_amd import _cabi
    from lanpaint_amd._util import raw_stream
    with torch.cuda.device(DEV):
        _cabi.check(getattr(_cabi.load(), entry)(ctypes.byref(desc), raw_stream(DEV)), entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("out_hw", [(8, 12), (16, 20)])
@pytest.mark.parametrize("c", [1, 3])
def test_device_origin_tables_are_clamped_in_both_resample_entries(c, out_hw):
    """The regions and track entries, and lp_detail_resample_subjects, whose table is indexed by the block itself."""
    from lanpaint_amd import _cabi
    assert _clamped(_CLAMP_ORIGINS) == ((0, 0), (15, 19), (5, 7))
    assert _clamped(_CLAMP_SUBJECT_ORIGINS)[3:] == ((2, 0), (0, 19), (15, 9))
    (h, w), (oh, ow), B = _CLAMP_WIN, out_hw, 3
    _, src = _guarded(B, _CLAMP_H, _CLAMP_W, c, seed=61)
    tables = (_axis_tables(w, ow), _axis_tables(h, oh)) if out_hw != _CLAMP_WIN else None

    def run(entry, origins):
        table = torch.tensor(origins, dtype=torch.int32, device=DEV)
        groups = {"lp_detail_resample_regions": len(origins), "lp_detail_resample_subjects": len(origins) // B}.get(entry, 1)
        whole, dst = _guarded(groups * B, oh, ow, c)
        if entry == "lp_detail_resample_regions":
            d = _cabi.LpDetailResampleRegionsDesc(B, _CLAMP_H, _CLAMP_W, c, groups, h, w, 0, oh, ow)
        elif entry == "lp_detail_resample_subjects":
            d = _cabi.LpDetailResampleSubjectsDesc(B, _CLAMP_H, _CLAMP_W, c, groups, h, w, 0, oh, ow)
        else:
            d = _cabi.LpDetailResampleTrackDesc(B, _CLAMP_H, _CLAMP_W, c, h, w, oh, ow)
        d.origins, d.src, d.dst = table.data_ptr(), src.data_ptr(), dst.data_ptr()
        if tables:
            (bx, wx), (by, wy) = tables
            d.ksize_x, d.ksize_y = wx.shape[1], wy.shape[1]
            d.bounds_x, d.weights_x, d.bounds_y, d.weights_y = bx.data_ptr(), wx.data_ptr(), by.data_ptr(), wy.data_ptr()
        _raw(entry, d)
        assert bool((whole[0] == _GUARD).all()) and bool((whole[-1] == _GUARD).all()), entry
        assert bool((dst != _GUARD).all()), entry                        # every element of every window was written
        return whole

    for entry, origins in (("lp_detail_resample_regions", _CLAMP_ORIGINS), ("lp_detail_resample_track", _CLAMP_ORIGINS),
                           ("lp_detail_resample_subjects", _CLAMP_SUBJECT_ORIGINS)):
        assert torch.equal(run(entry, origins), run(entry, _clamped(origins))), entry


@pytest.mark.parametrize("k", [1, 17])
@pytest.mark.parametrize("c", [1, 3])
def test_device_origin_table_is_clamped_in_the_track_stitch(c, k):
    from lanpaint_amd import _cabi
    (h, w), B = _CLAMP_WIN, 3
    _, original = _guarded(B, _CLAMP_H, _CLAMP_W, c, seed=62)
    _, mask = _guarded(B, _CLAMP_H, _CLAMP_W, seed=63)
    detail_img = (torch.rand(B, h, w, c, generator=_gen(64)) + 2.0).to(DEV)      # [2, 3): a blended element differs from the original

    def run(origins):
        table = torch.tensor(origins, dtype=torch.int32, device=DEV)
        whole, out = _guarded(B, _CLAMP_H, _CLAMP_W, c)
        d = _cabi.LpDetailStitchTrackDesc(B, _CLAMP_H, _CLAMP_W, c, h, w, k, B, table.data_ptr(), mask.data_ptr(),
                                          original.data_ptr(), detail_img.data_ptr(), out.data_ptr())
        _raw("lp_detail_stitch_track", d)
        assert bool((whole[0] == _GUARD).all()) and bool((whole[-1] == _GUARD).all())
        return whole

    got, want = run(_CLAMP_ORIGINS), run(_clamped(_CLAMP_ORIGINS))
    assert torch.equal(got, want)
    inside = torch.zeros(B, _CLAMP_H, _CLAMP_W, dtype=torch.bool)
    for f, (y0, x0) in enumerate(_clamped(_CLAMP_ORIGINS)):
        inside[f, y0:y0 + h, x0:x0 + w] = True
    changed = (got[1:-1] != original).any(dim=-1).cpu()
    assert bool(changed.any()) and not bool((changed & ~inside).any())   # the blend happened, and only inside the clamped windows


@pytest.mark.parametrize("k", [1, 17])
@pytest.mark.parametrize("c", [1, 3])
def test_device_origin_table_is_clamped_in_the_subjects_stitch(c, k):
    from lanpaint_amd import _cabi
    (h, w), B, S = _CLAMP_WIN, 3, len(_CLAMP_SUBJECT_ORIGINS) // 3
    _, original = _guarded(B, _CLAMP_H, _CLAMP_W, c, seed=65)
    _, mask = _guarded(B, _CLAMP_H, _CLAMP_W, seed=66)
    detail_imgs = (torch.rand(S * B, h, w, c, generator=_gen(67)) + 2.0).to(DEV)  # [2, 3): a blended element differs from the original

    def run(origins):
        table = torch.tensor(origins, dtype=torch.int32, device=DEV)
        whole, out = _guarded(B, _CLAMP_H, _CLAMP_W, c)
        d = _cabi.LpDetailStitchSubjectsDesc(B, _CLAMP_H, _CLAMP_W, c, S, h, w, k, 0, 0, table.data_ptr(), mask.data_ptr(),
                                             original.data_ptr(), detail_imgs.data_ptr(), out.data_ptr())       # no labels
        _raw("lp_detail_stitch_subjects", d)
        assert bool((whole[0] == _GUARD).all()) and bool((whole[-1] == _GUARD).all())
        return whole

    got, want = run(_CLAMP_SUBJECT_ORIGINS), run(_clamped(_CLAMP_SUBJECT_ORIGINS))
    assert torch.equal(got, want)
    inside = torch.zeros(B, _CLAMP_H, _CLAMP_W, dtype=torch.bool)
    for i, (y0, x0) in enumerate(_clamped(_CLAMP_SUBJECT_ORIGINS)):                # subject 0's windows and subject 1's
        inside[i % B, y0:y0 + h, x0:x0 + w] = True
    changed = (got[1:-1] != original).any(dim=-1).cpu()
    assert bool(changed.any()) and not bool((changed & ~inside).any())   # the blend happened, and only inside the clamped windows
