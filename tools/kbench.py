#!/usr/bin/env python3
"""Kernel micro-benchmarks at the shapes RawFormer-S/B use in BASELINE configs 2-3 (GPU box only).

Each case runs through the C ABI (ops.*) with the library's own HIP-event bracket
(rf_profile_begin/end), so the figure is the kernel's time on its launch stream, without the
weight-repack helper that the operator-level entry points run first.

usage: python tools/kbench.py [conv1x1] [conv3x3] [dw] [attn] [flca] [dwt] [ssim] [sampler] [mcr_sampler] [mamba] [wfb] [ffab_bwd] [wmb_bwd] [--dim 32] [--batch 8] [--size 512]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bayer_low_light_image_enhancement_amd import _lib, harness, ops  # noqa: E402


def timed(fn, iters=10, warm=2):
    lib = _lib.load()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    lib.rf_profile_begin()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(lib.rf_profile_end(buf, len(buf)), "rf_profile_end")
    return [r for r in json.loads(buf.value.decode()) if not r["kernel"].startswith("pack")]


def report(tag, recs):
    for r in recs:
        us = r["ms"] / r["launches"] * 1e3
        tf = r["flops"] / max(r["ms"], 1e-9) / 1e9
        gb = r["bytes"] / max(r["ms"], 1e-9) / 1e6
        print(f"{tag:44s} {r['kernel']:28s} {us:9.1f} us  {tf:7.2f} TF/s  {gb:8.1f} GB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["conv1x1", "conv3x3", "dw", "attn", "flca", "dwt"])
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, d = a.batch, a.size, a.dim
    r = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for lvl in range(4):
        C, h = d << lvl, S >> lvl
        x = r(B, C, h, h)
        if "conv1x1" in a.what:
            lw, lb = r(C), r(C)
            report(f"L{lvl} qkv   {C}->{3*C} LN        {h}x{h}", timed(lambda: ops.conv1x1(x, r(3 * C, C, 1, 1), r(3 * C), ln_weight=lw, ln_bias=lb)))
            report(f"L{lvl} pw1   {C}->{2*C} LN        {h}x{h}", timed(lambda: ops.conv1x1(x, r(2 * C, C, 1, 1), r(2 * C), ln_weight=lw, ln_bias=lb)))
            report(f"L{lvl} proj  {C}->{C} +res       {h}x{h}", timed(lambda: ops.conv1x1(x, r(C, C, 1, 1), r(C), residual=x)))
            x2 = r(B, 2 * C, h, h)
            report(f"L{lvl} pw2   {2*C}->{C} +res      {h}x{h}", timed(lambda: ops.conv1x1(x2, r(C, 2 * C, 1, 1), r(C), residual=x)))
            report(f"L{lvl} cat   {C}+{C}->{C}         {h}x{h}", timed(lambda: ops.conv1x1(x, r(C, 2 * C, 1, 1), r(C), x2=x)))
            if lvl < 3:
                xs = r(B, 2 * C, h // 2, h // 2)
                report(f"L{lvl} convT {2*C}->{C} x4        {h//2}x{h//2}", timed(lambda: ops.conv_transpose2x2(xs, r(2 * C, C, 2, 2), r(C))))
        if "conv3x3" in a.what:
            report(f"L{lvl} conv3 {C}->{C} lrelu      {h}x{h}", timed(lambda: ops.conv3x3(x, r(C, C, 3, 3), r(C), act="lrelu")))
            if lvl < 3:
                report(f"L{lvl} down  {C}->{C//2} unshuf   {h}x{h}", timed(lambda: ops.conv3x3(x, r(C // 2, C, 3, 3), None, store="unshuffle")))
            if lvl == 0:
                report(f"L0 embed 4->{C}             {h}x{h}", timed(lambda: ops.conv3x3(r(B, 4, h, h), r(C, 4, 3, 3), r(C))))
                report(f"L0 out   {C}->12 shuffle     {h}x{h}", timed(lambda: ops.conv3x3(x, r(12, C, 3, 3), r(12), act="lrelu", store="shuffle")))
        if "dw" in a.what:
            x3 = r(B, 3 * C, h, h)
            report(f"L{lvl} dw    {3*C}               {h}x{h}", timed(lambda: ops.dwconv3x3(x3, r(3 * C, 1, 3, 3), r(3 * C))))
            x2 = r(B, 2 * C, h, h)
            report(f"L{lvl} dw+gelu {2*C}             {h}x{h}", timed(lambda: ops.dwconv3x3(x2, r(2 * C, 1, 3, 3), r(2 * C), gelu=True)))
        if "attn" in a.what:
            report(f"L{lvl} chan_attn C={C}           {h}x{h}", timed(lambda: ops.channel_attention(
                x, r(3 * C, C, 1, 1), r(3 * C), r(3 * C, 1, 3, 3), r(3 * C), r(8, 1, 1), r(C, C, 1, 1), r(C), 8)))
    if "c3probe" in a.what:   # conv3x3 at controlled (Cin, Cout, size, batch): separates chunk count from image size
        for ci, co, sz, bb in ((32, 32, 512, 8), (64, 32, 512, 8), (32, 32, 256, 32), (32, 32, 1024, 2), (64, 32, 256, 8),
                               (16, 32, 512, 8), (32, 64, 512, 8), (64, 64, 512, 4)):
            xx = r(bb, ci, sz, sz)
            report(f"c3 {ci}->{co} {sz}x{sz} B={bb}", timed(lambda: ops.conv3x3(xx, r(co, ci, 3, 3), r(co), act="lrelu")))
            del xx
    if "ssim" in a.what:   # harness SSIM: a full SID frame and a batch of 8 x 1024 x 1024 (GB/s = the 2 B / element of algorithmic traffic)
        for bb, hh, ww in ((1, 2848, 4256), (8, 1024, 1024)):
            ia = torch.randint(0, 256, (bb, hh, ww, 3), dtype=torch.uint8, device=dev)
            ib = (ia.to(torch.int16) + torch.randint(-9, 10, ia.shape, dtype=torch.int16, device=dev)).clamp(0, 255).to(torch.uint8)
            report(f"ssim {bb}x{hh}x{ww}x3", timed(lambda: harness.ssim_u8_channel_means(ia, ib)))
            del ia, ib
    if "sampler" in a.what:   # training batch assembly: 16 patches of 512 x 512 out of 16 resident SID frames (GB/s = the 24 B / pixel of algorithmic traffic)
        from bayer_low_light_image_enhancement_amd.data import PatchSampler, ResidentSID
        nf, hh, ww = 16, 2848, 4256
        u16 = lambda *s: torch.randint(-32768, 32768, s, dtype=torch.int16, device=dev).view(torch.uint16)  # noqa: E731
        smp = PatchSampler(ResidentSID(u16(nf, hh, ww), u16(nf, hh, ww, 3), [100.0, 300.0] * (nf // 2)), patch_size=512, seed=0)
        report(f"sid_sample 16x512x512 of {nf}x{hh}x{ww}", timed(lambda: smp.batch(list(range(16)))))
        del smp
    if "mcr_sampler" in a.what:   # the same from 16 resident MCR frames (1024 x 1280 uint8; GB/s = the 20 B / pixel of algorithmic traffic)
        from bayer_low_light_image_enhancement_amd.data import PatchSampler, ResidentMCR
        nf, hh, ww = 16, 1024, 1280
        u8 = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device=dev)  # noqa: E731
        smp = PatchSampler(ResidentMCR(u8(nf, hh, ww), u8(nf, hh, ww, 3), [12287 / 255, 1023 / 255] * (nf // 2)), patch_size=512, seed=0)
        report(f"mcr_sample 16x512x512 of {nf}x{hh}x{ww}", timed(lambda: smp.batch(list(range(16)))))
        del smp
    if "mamba" in a.what:   # ops.wm on the high bands of the headline batch (n = 3 x 8) at level 0 and level 3 of the WFB U-Net.  The scan rows'
        # GB/s are algorithmic HBM bytes: mamba_scan_kernel<true> reads delta, x, z, Bm, Cm and writes y.  The chunk length is a build-time
        # constant: compare libraries built with -DRF_MAMBA_LC=<n> through RF_LIB_PATH (the figure in use is printed).
        print(f"rf_mamba_chunk_len() = {_lib.load().rf_mamba_chunk_len()}", flush=True)
        for n, c, hw in ((24, 32, 256), (24, 256, 32)):
            xw = r(n, c, hw, hw)
            shapes = {"convb.0.weight": (2 * c, c, 3, 3), "convb.0.bias": (2 * c,), "convb.2.weight": (c, 2 * c, 3, 3), "convb.2.bias": (c,),
                      "ln.weight": (c,), "ln.bias": (c,), "smooth.weight": (c, c, 3, 3), "smooth.bias": (c,)}
            shapes.update({"model1." + k: v for k, v in ops.mamba_param_shapes(c).items()})
            pw = {k: 0.1 * r(*v) for k, v in shapes.items()}
            pw["model1.A_log"] = torch.log(torch.arange(1, 33, device=dev, dtype=torch.float32)).repeat(2 * c, 1).contiguous()
            pw["model1.dt_proj.bias"] = torch.full((2 * c,), -4.0, device=dev)      # delta around 0.02
            recs = timed(lambda: ops.wm(xw, pw))
            report(f"wm n={n} c={c} {hw}x{hw}", recs)
            print(f"wm n={n} c={c} {hw}x{hw}: {sum(q['ms'] for q in recs) / 10:.3f} ms per call "
                  f"(sum of its kernels)", flush=True)
            del xw, pw
    if "wfb" in a.what:   # one forward of RawFormer(variant='wfb') at --dim on a --size mosaic, batch 1 and --batch: the handle (weights folded
        # and packed once, fused front / back / tail passes) against the same forward composed from ops.* (every call folds and packs
        # its own weights).  HIP-event brackets around `iters` forwards, both orders in one visit; then the handle's per-kernel table
        # (one stream while profiling) and the share of WM's 3x3 convolutions, from ops.wm at every level's shape.
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import wfb_ref
        from bayer_low_light_image_enhancement_amd import RawFormer
        m = RawFormer(dim=d, variant="wfb").to(dev).eval()
        pw = {k: v for k, v in m.state_dict().items() if v.dtype.is_floating_point}

        def event_ms(fn, iters=10, warm=2):
            for _ in range(warm):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        for bb in (1, B):
            xm = torch.rand(bb, 1, S, S, device=dev)
            with torch.no_grad():
                handle, composed = (lambda: m(xm)), (lambda: wfb_ref.ops_forward(pw, xm))
                t = [event_ms(handle), event_ms(composed), event_ms(composed), event_ms(handle)]
                print(f"wfb dim {d} mosaic {bb}x{S}x{S}: handle {t[0]:.3f} / {t[3]:.3f} ms, composed from ops.* {t[1]:.3f} / {t[2]:.3f} ms per forward "
                      f"(order: handle, composed, composed, handle); handle / composed = {(t[0] + t[3]) / (t[1] + t[2]):.3f}", flush=True)
                recs = timed(handle)
            total = sum(q["ms"] for q in recs)
            print(f"wfb handle {bb}x{S}x{S}: {sum(q['launches'] for q in recs) // 10} kernel launches per forward", flush=True)
            for q in sorted(recs, key=lambda q: -q["ms"]):      # per forward: launches, total time and share, then the per-launch figures
                print(f"wfb handle {bb}x{S}x{S}  {q['kernel']:40s} {q['launches'] // 10:5d} launches {q['ms'] / 10:8.3f} ms {100 * q['ms'] / total:5.1f} %  "
                      f"{q['ms'] / q['launches'] * 1e3:8.1f} us each  {q['bytes'] / max(q['ms'], 1e-9) / 1e6:8.1f} GB/s", flush=True)
            print(f"wfb handle {bb}x{S}x{S}: {total / 10:.3f} ms per forward as the sum of its kernels on one stream", flush=True)
            wm_ms, wm_conv = 0.0, 0.0
            for lvl in range(4):
                c, hw = d << lvl, (S // 2 >> lvl) // 2
                pre = f"conv_tran{lvl + 1}.Transformer.mb."
                sub = {k[len(pre):]: v for k, v in pw.items() if k.startswith(pre)}
                xw = r(3 * bb, c, hw, hw)
                rw = timed(lambda: ops.wm(xw, sub))
                ms, cv = sum(q["ms"] for q in rw) / 10, sum(q["ms"] for q in rw if "conv3x3" in q["kernel"]) / 10
                n_stage = 1 if lvl == 3 else 2
                wm_ms, wm_conv = wm_ms + n_stage * ms, wm_conv + n_stage * cv
                print(f"  wm level {lvl} n={3 * bb} c={c} {hw}x{hw}: {ms:.3f} ms, 3x3 convolutions {cv:.3f} ms ({100 * cv / ms:.0f} %)", flush=True)
            print(f"wfb {bb}x{S}x{S}: WM over the 7 stages {wm_ms:.3f} ms = {100 * wm_ms / (total / 10):.0f} % of the forward's kernel time; "
                  f"its 3x3 convolutions {wm_conv:.3f} ms = {100 * wm_conv / wm_ms:.0f} % of WM", flush=True)
            del xm
    if "ffab_bwd" in a.what:   # ops.ffab_backward against ops.ffab on the LL band of four 512 x 512 patches at level 0 and level 3 of RawFormer-S:
        # HIP events around `iters` calls, both orders in one visit (workspace allocation and the per-call weight packs included, for
        # both); then the backward's per-kernel table on one stream and the share of the four transform-adjoint kernels
        def event_ms(fn, iters=10, warm=2):
            for _ in range(warm):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        for bb, c, hw in ((4, 32, 128), (4, 256, 16)):
            xf, gf = torch.rand(bb, c, hw, hw, device=dev) * 2 - 1, r(bb, c, hw, hw)
            pf = {k: (torch.rand(*v, device=dev) * 2 - 1) / (v[1] if len(v) == 4 else v[0]) ** 0.5 for k, v in ops.ffab_param_shapes(c).items()}
            fwd, bwd = (lambda: ops.ffab(xf, pf)), (lambda: ops.ffab_backward(xf, pf, gf))
            t = [event_ms(fwd), event_ms(bwd), event_ms(bwd), event_ms(fwd)]
            print(f"ffab ({bb},{c},{hw},{hw}): forward {t[0]:.3f} / {t[3]:.3f} ms, backward {t[1]:.3f} / {t[2]:.3f} ms per call (order: forward, "
                  f"backward, backward, forward); backward / forward = {(t[1] + t[2]) / (t[0] + t[3]):.2f}", flush=True)
            for tag, fn in (("forward", fwd), ("backward", bwd)):
                recs = timed(fn)
                total = sum(q["ms"] for q in recs)
                for q in sorted(recs, key=lambda q: -q["ms"]):
                    print(f"ffab {tag} ({bb},{c},{hw},{hw})  {q['kernel']:40s} {q['launches'] // 10:5d} launches {q['ms'] / 10:8.3f} ms {100 * q['ms'] / total:5.1f} %  "
                          f"{q['ms'] / q['launches'] * 1e3:8.1f} us each  {q['bytes'] / max(q['ms'], 1e-9) / 1e6:8.1f} GB/s", flush=True)
                adj = sum(q["ms"] for q in recs if q["kernel"].endswith("_backward(2 kernels)"))
                print(f"ffab {tag} ({bb},{c},{hw},{hw}): {total / 10:.3f} ms per call as the sum of its bracketed kernels on one stream"
                      + (f"; the four transform-adjoint kernels {adj / 10:.3f} ms = {100 * adj / total:.1f} %" if tag == "backward" else ""), flush=True)
            del xf, gf, pf
    if "wmb_bwd" in a.what:   # the WMB backward pieces at level 0 and level 3 of RawFormer-S at the training patch, given as the
        # full-resolution shape: HIP events around 4 calls per sample, 15 rounds that take one sample of every candidate in turn after
        # 3 warm-up calls each; median (min - max) in ms per call.  front: the fused kernel against the same function composed from
        # ops.iwt_init + rf_affine_clamp_add + ops.layernorm2d_backward; back and illumination: against their forward operators
        import statistics

        def rounds(cands, calls=4, n=15, warm=3):
            for fn in cands.values():
                for _ in range(warm):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in cands}
            for _ in range(n):
                for k, fn in cands.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        fn()
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / calls)
            return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

        lib = _lib.load()
        for bb, c, hh, ww in ((4, 32, 256, 256), (4, 256, 32, 32)):
            u = lambda *s: torch.rand(*s, device=dev) * 2 - 1  # noqa: E731
            xf, gt, gb = u(bb, c, hh, ww) * 2, u(bb, c, hh, ww), u(4 * bb, c, hh // 2, ww // 2)
            w2, b2 = 2 * (u(c) * 0.5 + 1), u(c)
            bands = u(4 * bb, c, hh // 2, ww // 2) * 2

            def composed():
                g = ops.iwt_init(gb)
                _lib.check(lib.rf_affine_clamp_add(g.data_ptr(), gt.data_ptr(), g.data_ptr(), g.numel(), 1.0, 0.0, float("-inf"), float("inf"), None),
                           "rf_affine_clamp_add")
                return ops.layernorm2d_backward(xf, w2, g)

            ch, cw = hh // 2, ww // 2
            img, gfea = u(bb, c, ch, cw), u(bb, c, ch, cw)
            pi = {"conv1.weight": u(c, c + 1, 1, 1) / c ** 0.5, "conv1.bias": u(c), "depth_conv.weight": u(c, 1, 5, 5) / 5, "depth_conv.bias": u(c),
                  "conv2.weight": u(c, c, 1, 1) / c ** 0.5, "conv2.bias": u(c)}
            res = rounds({"front fused": lambda: ops.wmb_front_backward(xf, w2, b2, gt, gb, grad_scale=2.0), "front composed": composed,
                          "back backward": lambda: ops.wmb_back_backward(bands, gt), "back forward": lambda: ops.wmb_back(bands, gt),
                          "illumination backward": lambda: ops.illumination_estimator_backward(img, pi, gfea),
                          "illumination forward": lambda: ops.illumination_estimator(img, pi)})
            for k, (med, lo, hi) in res.items():
                print(f"wmb_bwd ({bb},{c},{hh},{ww})  {k:24s} {med:8.4f} ms  ({lo:.4f} - {hi:.4f})", flush=True)
            el = bb * c * hh * ww
            print(f"wmb_bwd ({bb},{c},{hh},{ww})  front fused / composed = {res['front fused'][0] / res['front composed'][0]:.3f}; fused "
                  f"{16 * el / res['front fused'][0] / 1e6:.0f} GB/s of its 16 B / element; back backward / forward = "
                  f"{res['back backward'][0] / res['back forward'][0]:.3f} ({12 * el / res['back backward'][0] / 1e6:.0f} GB/s of 12 B / element); "
                  f"illumination backward / forward = {res['illumination backward'][0] / res['illumination forward'][0]:.3f}", flush=True)
            for tag, fn in (("front fused", lambda: ops.wmb_front_backward(xf, w2, b2, gt, gb, grad_scale=2.0)),
                            ("illumination backward", lambda: ops.illumination_estimator_backward(img, pi, gfea))):
                report(f"wmb_bwd ({bb},{c},{hh},{ww}) {tag}", timed(fn))
    if "dwt" in a.what:
        x = r(B, d, S, S)
        report("dwt_init", timed(lambda: ops.dwt_init(x)))
        report("iwt_init", timed(lambda: ops.iwt_init(x.reshape(4 * B, d // 4, S, S))))
        report("CustomDWT", timed(lambda: ops.custom_dwt(x)))
        report("CustomIDWT", timed(lambda: ops.custom_idwt(x)))
        report("downshuffle", timed(lambda: ops.downshuffle(x)))
        report("pixel_shuffle", timed(lambda: ops.pixel_shuffle(x)))
        report("layernorm2d", timed(lambda: ops.layernorm2d(x, r(d), r(d))))


if __name__ == "__main__":
    main()
