"""Stand-ins for the ComfyUI pieces the AV nodes touch -- comfy.nested_tensor, comfy_api's video types, a source VIDEO -- and
two small deterministic VAEs (fixed linear maps).  Shared by tests/golden/make_av_golden.py, which runs the reference's
nodes through them, and the tests, which run lanpaint_amd.av_nodes through the same ones."""
from __future__ import annotations

import contextlib
import sys
import types

import numpy as np
import torch


class NestedTensor:
    """comfy.nested_tensor.NestedTensor as far as the nodes use it: built from a tuple, `is_nested`, `unbind()`."""
    is_nested = True

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def unbind(self):
        return tuple(self.tensors)


class VideoComponents:
    def __init__(self, images, audio=None, frame_rate=None):
        self.images, self.audio, self.frame_rate = images, audio, frame_rate


class VideoFromComponents:
    def __init__(self, components, bit_depth=None):
        self.components, self.bit_depth = components, bit_depth

    def get_components(self):
        return self.components


class SourceVideo:
    """A VIDEO input: frames [F, H, W, 3] in 0..1 and an optional AUDIO dict."""

    def __init__(self, images, audio, frame_rate=5, bit_depth=8):
        self._c = VideoComponents(images, audio, frame_rate)
        self._bit_depth = bit_depth

    def get_components(self):
        return self._c

    def get_frame_rate(self):
        return self._c.frame_rate

    def get_bit_depth(self):
        return self._bit_depth


class StubVideoVAE:
    """encode [F, H, W, 3] -> [1, 3, F, H/2, W/2] (2x2 means); decode -> [1, F, 2h + 2, 2w, 3]: nearest x2, two repeated
    rows (so the node has to resize back) and a fixed affine colour map."""

    def encode(self, px):
        f, h, w, c = px.shape
        x = px.permute(3, 0, 1, 2).reshape(1, c, f, h // 2, 2, w // 2, 2)
        return x.mean(dim=(4, 6))

    def decode(self, z):
        y = z.repeat_interleave(2, dim=-1).repeat_interleave(2, dim=-2)
        y = torch.cat([y, y[..., -2:, :]], dim=-2)
        return (0.9 - 0.8 * y).permute(0, 2, 3, 4, 1)


class StubAudioVAE:
    """channels-last in and out, like the MiniMax H3 wrapper: encode [B, L, C] -> [B, C, L/4] (means of 4), decode
    [B, C, T] -> [B, 4T - 3, C] (repeat x4, affine, the last 3 samples dropped: the merge has to cut to the shorter)."""
    audio_sample_rate = 800

    def encode(self, x):
        b, l, c = x.shape
        return x.movedim(-1, 1).reshape(b, c, l // 4, 4).mean(dim=-1)

    def decode(self, z):
        y = 0.5 * z.repeat_interleave(4, dim=-1) + 0.1
        return y[..., :-3].movedim(1, -1)


def node_inputs(seed=11):
    """The source video (6 frames of 14 x 18 at 5 fps, 1.2 s of mono audio at 800 Hz) and the two masks."""
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.random((6, 14, 18, 3), dtype=np.float32))
    wave = torch.from_numpy((0.3 * rng.standard_normal((1, 1, 960))).astype(np.float32))
    mask = torch.zeros(6, 14, 18)
    mask[1:4, 3:10, 5:14] = 1.0
    audio_mask = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    video = SourceVideo(frames, {"waveform": wave, "sample_rate": 800})
    return video, mask, audio_mask


@contextlib.contextmanager
def comfy_modules(extra=()):
    """comfy, comfy.nested_tensor and comfy_api's two video-type modules in sys.modules for the block, then the previous
    entries back.  `extra`: more (name, module) pairs installed the same way."""
    comfy = types.ModuleType("comfy")
    comfy.__path__ = []
    nested = types.ModuleType("comfy.nested_tensor")
    nested.NestedTensor = NestedTensor
    comfy.nested_tensor = nested
    mods = {"comfy": comfy, "comfy.nested_tensor": nested}
    for name in ("comfy_api", "comfy_api.latest", "comfy_api.latest._input_impl", "comfy_api.latest._util"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    inp = types.ModuleType("comfy_api.latest._input_impl.video_types")
    inp.VideoFromComponents = VideoFromComponents
    inp.VideoFromFile = None
    util = types.ModuleType("comfy_api.latest._util.video_types")
    util.VideoComponents = VideoComponents
    mods["comfy_api.latest._input_impl.video_types"], mods["comfy_api.latest._util.video_types"] = inp, util
    for name, mod in extra:
        mods[name] = mod
    for name, mod in list(mods.items()):           # the attribute chain a dotted import walks
        parent, _, leaf = name.rpartition(".")
        if parent in mods:
            setattr(mods[parent], leaf, mod)
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        yield mods
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
