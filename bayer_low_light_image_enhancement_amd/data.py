"""Training batches from a device-resident SID or MCR set (RawFomer_WFB_FFAB/load_dataset.py:9-179).

The reference keeps the decoded Sony split in host memory as uint16 arrays (``image_read_SID``, :9-31) and cuts, flips and
normalises one patch per item in its loader workers (``load_data_SID.__getitem__``, :53-95).  Here the same arrays live in
device memory (``ResidentSID``; the training split is about 16 GB), the host draws only the four random numbers of a patch
(``PatchSampler``, the reference's draw order on a private ``random.Random``) and one kernel (``rf_sid_sample``,
``csrc/rf_sampler.hip``) assembles the whole batch, bit for bit what ``__getitem__`` returns.

The Mono-Colored-RAW set (``image_read_MCR`` / ``load_data_MCR``, :97-179) goes the same way: ``ResidentMCR`` holds the uint8
colour-raw frames and RGB targets as ``imageio`` returns them and the float64 exposure ratio of every frame
(``mcr_amp_from_names``, the reference's file-name slices), ``rf_mcr_sample`` restates ``(inp / 255 * amp).astype(float32)`` in
float64 with one rounding, and the same ``PatchSampler`` serves both sets: the two ``__getitem__`` bodies draw identically.

As in the reference the flips are flips of the MOSAIC: a left-right flip of an even-aligned crop moves the CFA phase by one
column, an up-down flip by one row.  That is the reference's augmentation and is reproduced, not corrected.

Decoding the files (rawpy for SID's ARW, imageio for MCR's tif / jpg) stays with the caller.
"""
from __future__ import annotations

import ctypes as C
import random
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def amp_from_names(paths: Iterable[str]) -> List[float]:
    """The amplification of every item from its LONG exposure's file name (:81-84): 300 where ``path[-7] == '3'``
    (``..._30s.ARW`` beside a 0.1 s short exposure), 100 otherwise."""
    return [300.0 if p[-7] == "3" else 100.0 for p in paths]


def mcr_amp_from_names(paths: Iterable[str]) -> List[float]:
    """The exposure ratio of every MCR item from its colour-raw file name (``load_data_MCR.__getitem__``, :141-149), e.g.
    ``.../C00012_48mp_0x8_0x00ff.tif``: ``img_num = int(p[-23:-20])``, ``img_expo = int(p[-8:-4], 16)``, ``gt_expo`` 12287 below
    image number 500 and 1023 from there on, ``amp = gt_expo / img_expo`` as a Python float (float64)."""
    out = []
    for p in paths:
        try:
            if len(p) < 23:
                raise ValueError("shorter than the 23 characters the slices reach back")
            img_num = int(p[-23:-20])
            img_expo = int(p[-8:-4], 16)
        except ValueError as e:
            raise ValueError(f"mcr_amp_from_names: cannot parse {p!r}: {e}") from None
        if img_expo == 0:
            raise ValueError(f"mcr_amp_from_names: {p!r}: exposure 0")
        out.append((12287 if img_num < 500 else 1023) / img_expo)
    return out


_EXACT = {torch.uint16: np.uint16, torch.uint8: np.uint8}          # the frames: no silent conversion


def _device_tensor(a, dtype, what: str, device, who: str = "ResidentSID") -> torch.Tensor:
    name = str(dtype).split(".")[1]
    if isinstance(a, np.ndarray):
        if dtype in _EXACT and a.dtype != _EXACT[dtype]:
            raise TypeError(f"{who}: {what} must be {name}, got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a))
    elif not isinstance(a, torch.Tensor):
        a = torch.as_tensor(a, dtype=None if dtype in _EXACT else dtype)
    if dtype in _EXACT:
        if a.dtype != dtype:
            raise TypeError(f"{who}: {what} must be {name}, got {a.dtype}")
    else:
        a = a.to(dtype)
    return a.to(device).contiguous()


class ResidentSID:
    """The decoded set in device memory: ``raw`` uint16 ``[N,H,W]`` (``raw_image_visible``), ``gt`` uint16 ``[N,H,W,3]``
    (``postprocess(..., output_bps=16)``, HWC as rawpy returns it) and ``amp`` float32 ``[N]``.  numpy arrays and tensors
    are accepted; host data is copied to ``device`` (default: the current ROCm device), device tensors are used in place."""

    def __init__(self, raw_u16, gt_u16, amp, black: int = 512, white: int = 16383, device=None):
        if device is None:
            device = raw_u16.device if isinstance(raw_u16, torch.Tensor) and raw_u16.is_cuda else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ResidentSID keeps the set on a ROCm device: there is no CPU path in this package")
        self.raw = _device_tensor(raw_u16, torch.uint16, "raw", device)
        self.gt = _device_tensor(gt_u16, torch.uint16, "gt", device)
        self.amp = _device_tensor(amp, torch.float32, "amp", device)
        if self.raw.dim() != 3:
            raise ValueError(f"ResidentSID: raw must be [N,H,W], got {tuple(self.raw.shape)}")
        n, h, w = self.raw.shape
        if tuple(self.gt.shape) != (n, h, w, 3):
            raise ValueError(f"ResidentSID: gt must be {(n, h, w, 3)} (HWC), got {tuple(self.gt.shape)}")
        if tuple(self.amp.shape) != (n,):
            raise ValueError(f"ResidentSID: amp must be {(n,)}, got {tuple(self.amp.shape)}")
        if w % 2:
            raise ValueError(f"ResidentSID: frame width {w} must be even")
        if not 0 <= int(black) < int(white):
            raise ValueError(f"ResidentSID: black level {black}, white level {white}")
        self.n, self.h, self.w = n, h, w
        self.black, self.white = int(black), int(white)
        self.device = device

    amp_from_names = staticmethod(amp_from_names)

    def __len__(self) -> int:
        return self.n

    def _sample(self, table: torch.Tensor, x: torch.Tensor, gt: torch.Tensor, b: int, ph: int, pw: int) -> None:
        _lib.launch("rf_sid_sample", x, self.raw, self.gt, self.amp, table, x, gt, self.n, self.h, self.w, b, ph, pw, self.black, self.white)


class ResidentMCR:
    """The decoded Mono-Colored-RAW set in device memory: ``raw`` uint8 ``[N,H,W]`` (the colour-raw tif), ``gt`` uint8 ``[N,H,W,3]``
    (the RGB target, HWC as imageio returns it) and ``amp`` float64 ``[N]`` (``mcr_amp_from_names``).  numpy arrays and tensors
    are accepted; host data is copied to ``device`` (default: the current ROCm device), device tensors are used in place."""

    def __init__(self, raw_u8, gt_u8, amp, device=None):
        if device is None:
            device = raw_u8.device if isinstance(raw_u8, torch.Tensor) and raw_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ResidentMCR keeps the set on a ROCm device: there is no CPU path in this package")
        self.raw = _device_tensor(raw_u8, torch.uint8, "raw", device, "ResidentMCR")
        self.gt = _device_tensor(gt_u8, torch.uint8, "gt", device, "ResidentMCR")
        self.amp = _device_tensor(amp, torch.float64, "amp", device, "ResidentMCR")
        if self.raw.dim() != 3:
            raise ValueError(f"ResidentMCR: raw must be [N,H,W], got {tuple(self.raw.shape)}")
        n, h, w = self.raw.shape
        if tuple(self.gt.shape) != (n, h, w, 3):
            raise ValueError(f"ResidentMCR: gt must be {(n, h, w, 3)} (HWC), got {tuple(self.gt.shape)}")
        if tuple(self.amp.shape) != (n,):
            raise ValueError(f"ResidentMCR: amp must be {(n,)}, got {tuple(self.amp.shape)}")
        if w % 2:
            raise ValueError(f"ResidentMCR: frame width {w} must be even")
        self.n, self.h, self.w = n, h, w
        self.device = device

    amp_from_names = staticmethod(mcr_amp_from_names)

    def __len__(self) -> int:
        return self.n

    def _sample(self, table: torch.Tensor, x: torch.Tensor, gt: torch.Tensor, b: int, ph: int, pw: int) -> None:
        _lib.launch("rf_mcr_sample", x, self.raw, self.gt, self.amp, table, x, gt, self.n, self.h, self.w, b, ph, pw)


class PatchSampler:
    """``load_data_SID.__getitem__`` / ``load_data_MCR.__getitem__`` (``dataset``: a ``ResidentSID`` or a ``ResidentMCR``) for a list of
    indices at once.  The descriptors (frame, i, j, flips) are drawn on the host
    from a private ``random.Random(seed)`` in the reference's order per item -- ``randint(0, (H - P - 2) // 2) * 2`` for i, the same
    for j, ``randint(0, 100) > 50`` (left-right), ``randint(0, 100) < 20`` (up-down) -- so the same seed and index list give the
    patches the reference's dataset gives after ``random.seed(seed)``.  ``patch_size``: P (the reference's square patches) or
    ``(ph, pw)``."""

    def __init__(self, dataset, patch_size=512, seed=None):
        ph, pw = (int(v) for v in patch_size) if isinstance(patch_size, (tuple, list)) else (int(patch_size), int(patch_size))
        if ph <= 0 or pw <= 0 or pw % 4:
            raise ValueError(f"PatchSampler: patch size {patch_size}: the width must be a positive multiple of 4")
        if dataset.h - ph - 2 < 0 or dataset.w - pw - 2 < 0:
            raise ValueError(f"PatchSampler: frames of {dataset.h}x{dataset.w} are too small for patches of {ph}x{pw} (the reference draws from H - P - 2)")
        self.dataset, self.patch_size, self.ph, self.pw = dataset, patch_size, ph, pw
        self.rng = random.Random(seed)

    def draw(self, indices: Sequence[int]) -> List[Tuple[int, int, int, int]]:
        """The next descriptor ``(frame, i, j, flips)`` of every index; flips bit 0 = left-right, bit 1 = up-down."""
        d, out = self.dataset, []
        for idx in indices:
            i = self.rng.randint(0, (d.h - self.ph - 2) // 2) * 2
            j = self.rng.randint(0, (d.w - self.pw - 2) // 2) * 2
            lr = self.rng.randint(0, 100) > 50
            ud = self.rng.randint(0, 100) < 20
            out.append((int(idx), i, j, int(lr) | int(ud) << 1))
        return out

    def gather(self, desc: Sequence[Sequence[int]], ph: int, pw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The patches of an explicit descriptor table: ``x [B,1,ph,pw]``, ``gt [B,3,ph,pw]`` (float32, on the current stream)."""
        d = self.dataset
        b = len(desc)
        table = np.ascontiguousarray(np.asarray(desc, dtype=np.int64).reshape(b, 4).astype(np.int32))
        _lib.call("rf_sid_check_desc", table.ctypes.data_as(C.POINTER(C.c_int)), d.n, d.h, d.w, b, ph, pw)
        dev_table = torch.from_numpy(table).to(d.device)
        x = torch.empty((b, 1, ph, pw), dtype=torch.float32, device=d.device)
        gt = torch.empty((b, 3, ph, pw), dtype=torch.float32, device=d.device)
        d._sample(dev_table, x, gt, b, ph, pw)
        return x, gt

    def batch(self, indices: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """Random patches of the items ``indices`` (``training=True``): ``x [B,1,P,P]``, ``gt [B,3,P,P]``."""
        return self.gather(self.draw(indices), self.ph, self.pw)

    def whole(self, indices: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The whole frames of the items ``indices`` (``training=False``, :77-79): no crop, no flip, no random draw."""
        d = self.dataset
        return self.gather([(int(i), 0, 0, 0) for i in indices], d.h, d.w)
