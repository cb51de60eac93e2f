"""ResNet-50 (v1.5) inference on aiko_services_amd's HIP kernels — NHWC bf16, BN folded.

Not present in the reference (which delegates every model to third-party libraries, SURVEY
§2.4 K12); it is the model of BASELINE config 2/3 and the bench headline.  Architecture as
torchvision ``resnet50``: 7x7/2 stem, 3x3/2 max-pool, bottleneck stages [3, 4, 6, 3] with the
stride on the 3x3 conv, global average pool, 2048 -> 1000 classifier.

Execution plan per forward (B frames, all on one HIP stream, graph-capturable):

  preprocess (u8 resize/normalise -> padded 4-ch)  -> stem igemm (+bias+ReLU)
  -> maxpool -> 16 bottlenecks (3 igemm convs each; the 3rd fuses bias + residual + ReLU,
     the projection shortcut is one more igemm) -> avgpool -> FC igemm -> softmax/top-k

Weights are random-init (no checkpoints offline) with deterministic seeds; BatchNorm running
statistics are random too and folded into the conv weights at construction.
"""
from __future__ import annotations

import os

import math
from dataclasses import dataclass

import torch

from ..ops import conv as C
from .weights import WeightsMixin
from ..ops import vision as V

STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))
EXPANSION = 4


def _rand_bn(g: torch.Generator, c: int, gamma_range=(0.5, 1.0)):
    lo, hi = gamma_range
    gamma = lo + (hi - lo) * torch.rand(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    mean = 0.1 * torch.randn(c, generator=g)
    var = 0.5 + torch.rand(c, generator=g)
    return gamma, beta, mean, var


def _rand_conv(g: torch.Generator, cout: int, cin: int, k: int) -> torch.Tensor:
    fan_in = cin * k * k
    return torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / fan_in)


# workgroups of the persistent stage-1 kernel: one per CU (fewer, to leave CUs to the other frame
# lane, measured as noise in round 5: profiles/bneck_r5.md)
_BN_GRID = 0


@dataclass
class Bottleneck:
    conv1: C.ConvSpec
    conv2: C.ConvSpec
    conv3: C.ConvSpec
    down: C.ConvSpec | None
    fused: C.ConvSpec | None = None   # conv3 + projection shortcut as one K-concatenated igemm


class ResNet50(WeightsMixin):
    """Packed ResNet-50 for inference.  ``forward(frames_u8) -> (top-k probs, top-k ids)``."""

    def __init__(self, num_classes: int = 1000, seed: int = 0, device="cuda", image_size=224,
                 topk: int = 5):
        self.device = torch.device(device)
        self.image_size = image_size
        self.num_classes = num_classes
        self.topk = topk
        g = torch.Generator().manual_seed(seed)
        w = _rand_conv(g, 64, 3, 7)
        wf, b = C.fold_bn(w, *_rand_bn(g, 64))
        self.stem = C.make_stem_spec(wf, b, act="relu", device=self.device)
        self.blocks: list[Bottleneck] = []
        cin = 64
        for width, nblocks, stride in STAGES:
            for i in range(nblocks):
                s = stride if i == 0 else 1
                cout = width * EXPANSION
                c1 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, width, cin, 1), *_rand_bn(g, width)),
                                      act="relu", device=self.device)
                c2 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, width, width, 3), *_rand_bn(g, width)),
                                      stride=s, pad=1, act="relu", device=self.device)
                # small gamma on the last BN keeps the random residual stream bounded
                c3 = C.make_conv_spec(*C.fold_bn(_rand_conv(g, cout, width, 1),
                                                 *_rand_bn(g, cout, (0.1, 0.3))),
                                      act="relu", device=self.device)
                down = None
                if i == 0:
                    down = C.make_conv_spec(*C.fold_bn(_rand_conv(g, cout, cin, 1), *_rand_bn(g, cout)),
                                            stride=s, act=None, device=self.device)
                fused = C.fuse_shortcut(c3, down) if down is not None else None
                self.blocks.append(Bottleneck(c1, c2, c3, down, fused))
                cin = cout
        fc_w = 0.01 * torch.randn(num_classes, 2048, generator=g)
        fc_b = torch.zeros(num_classes)
        self.fc = C.make_linear_spec(fc_w, fc_b, device=self.device)
        self._ws: dict = {}
        self.fuse_shortcut = True
        self.fuse_stem_pool = True       # stem conv + ReLU + max-pool in one kernel
        # Infinity-Cache blocking of the memory-bound early stages (see features_from_stem): off —
        # measured slower than the fused stage-1 kernels (profiles/mall_blocking_resnet50_r1.txt,
        # round-5 A/B); the attributes stay for the equivalence test
        self.mall_chunk = 0
        self.mall_blocks = 3
        # conv_chain: identity block's 1x1 expansion + next block's 1x1 reduction in one launch
        self.chain = os.environ.get("AIKO_RESNET_CHAIN", "1") != "0"
        # stage-1 bottlenecks as ONE launch each (bneck_fused.hip: t1 / t2 stay in LDS)
        self.bneck = os.environ.get("AIKO_RESNET_BNECK", "1") != "0"
        # stage-3 identity blocks: 3x3 conv + 1x1 expansion + residual as ONE launch
        # (conv_exp.hip: t2 stays in LDS)
        self.exp3 = os.environ.get("AIKO_RESNET_EXP", "1") != "0"
        # uint8 frames of the model's own size go straight into the fused stem (it normalises
        # while filling its LDS patch): no pre-processing kernel, no bf16 stem buffer
        self.stem_u8 = os.environ.get("AIKO_STEM_U8", "1") != "0"

    # ---- workspace: every activation buffer allocated once per batch size ----------------
    def _buf(self, key: str, shape, dtype=torch.bfloat16) -> torch.Tensor:
        k = (key, tuple(shape), dtype)
        t = self._ws.get(k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._ws[k] = t
        return t

    def release_workspace(self) -> None:
        self._ws.clear()

    def _fc_work(self, tag: str, B: int) -> torch.Tensor:
        """fp32 partials of the split-K classifier (ops.conv.linear), one buffer per tag (lane)."""
        return self._buf(tag + "fc_part", (C.LINEAR_SPLITK * B * self.num_classes,), torch.float32)

    # ---- forward ------------------------------------------------------------------------
    def preprocess(self, frames: torch.Tensor, tag: str = "") -> torch.Tensor:
        """uint8 [B, H, W, 3] (any H, W) -> zero-bordered bf16 stem buffer [B, Hp, Wp, 4]."""
        B = frames.shape[0]
        S = self.image_size
        Hp, Wp = C.stem_geometry(S, S)
        return V.preprocess_frames(frames, (S, S), out=self._buf(tag + "pre", (B, Hp, Wp, 4)))

    def _stem_u8_ok(self, frames: torch.Tensor) -> bool:
        S = self.image_size
        return (self.stem_u8 and self.fuse_stem_pool and frames.dtype == torch.uint8 and frames.dim() == 4
                and frames.shape[1] == S and frames.shape[2] == S and S % 4 == 0 and frames.is_contiguous())

    def features_from_frames(self, frames: torch.Tensor, tag: str = "", after_block=None) -> torch.Tensor:
        """uint8 frames -> pooled features: through the uint8 fused stem when the frames have
        the model's size, else pre-processing + :meth:`features_from_stem`."""
        if not self._stem_u8_ok(frames):
            return self.features_from_stem(self.preprocess(frames, tag), tag, after_block=after_block)
        return self.features_from_stem(None, tag, after_block=after_block, frames=frames)

    def features_from_stem(self, x: torch.Tensor | None, tag: str = "", after_block=None,
                           pooled: torch.Tensor | None = None,
                           frames: torch.Tensor | None = None) -> torch.Tensor:
        """Stem buffer -> pooled features bf16 [B, 2048].  ``after_block`` = (index, fn): call
        ``fn()`` once bottleneck ``index`` is enqueued (-1: after the max-pool).  ``pooled``: the
        stem + max-pool output already computed (``x`` unused); ``frames``: uint8 frames of the
        model's size for the uint8 fused stem (``x`` unused)."""
        if pooled is not None:
            B = pooled.shape[0]
            if after_block is not None and after_block[0] < 0:
                after_block[1]()
            x, t1 = pooled, None
            for bi in range(len(self.blocks)):
                x, t1 = self._block(bi, x, tag, B, 0, B, t1)
                if after_block is not None and after_block[0] == bi:
                    after_block[1]()
            return V.avgpool(x, out=self._buf(tag + "gap", (B, x.shape[3])))
        B = (frames if frames is not None else x).shape[0]
        S = self.image_size
        Ho, Wo = C.stem_out_hw(S, S)
        Hm, Wm = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
        # Infinity-Cache blocking: the stem and the first ``mall_blocks`` bottlenecks run per
        # sub-batch of ``mall_chunk`` frames (views of the full-batch buffers), so each block's
        # input, intermediates and output stay within the 256 MiB die-level cache between
        # producer and consumer instead of round-tripping HBM; later (compute-bound, small)
        # stages run on the whole batch.
        ch = self.mall_chunk if 0 < self.mall_chunk < B and B % self.mall_chunk == 0 else B
        nb = self.mall_blocks if ch < B else 0
        pool = self._buf(tag + "pool", (B, Hm, Wm, 64))
        xs = []
        for c0 in range(0, B, ch):
            if frames is not None:
                xc = C.stem_pool_u8(frames[c0:c0 + ch], self.stem, V.IMAGENET_MEAN, V.IMAGENET_STD,
                                    out=pool[c0:c0 + ch])
            elif self.fuse_stem_pool:
                xc = C.stem_pool(x[c0:c0 + ch], self.stem, (S, S), out=pool[c0:c0 + ch])
            else:
                xc = x[c0:c0 + ch]
                st = self._buf(tag + "stem", (B, Ho, Wo, 64))[c0:c0 + ch]
                xc = V.maxpool2d(C.conv2d(xc, self.stem, out=st, image_hw=(S, S)), 3, 2, 1, out=pool[c0:c0 + ch])
            t1 = None
            for bi in range(nb):
                xc, t1 = self._block(bi, xc, tag, B, c0, ch, t1, chain=bi + 1 < nb)
            xs.append(xc)
        if len(xs) == 1:
            x = xs[0]
        elif nb == 0:
            x = pool
        else:                                      # the full-batch buffer the slices went to
            x = self._buf(tag + ("xa" if (nb - 1) % 2 == 0 else "xb"), (B,) + tuple(xs[0].shape[1:]))
        if after_block is not None and after_block[0] < nb:
            after_block[1]()
        t1 = None
        for bi in range(nb, len(self.blocks)):
            x, t1 = self._block(bi, x, tag, B, 0, B, t1)
            if after_block is not None and after_block[0] == bi:
                after_block[1]()
        return V.avgpool(x, out=self._buf(tag + "gap", (B, x.shape[3])))

    def _block(self, bi: int, x: torch.Tensor, tag: str, B: int, c0: int, ch: int,
               t1: torch.Tensor | None = None, chain: bool = True):
        """Bottleneck ``bi`` on frames c0 .. c0+ch of the batch (slices of [B, ...] buffers).
        ``t1``: this block's conv1 output when the previous block already produced it.
        Returns (output, next block's conv1 output or None): an identity block whose expansion
        conv3 feeds a 1x1 reduction runs both as one ``conv_chain`` launch."""
        blk = self.blocks[bi]
        H, W = x.shape[1], x.shape[2]
        sl = slice(c0, c0 + ch)
        conv3 = blk.fused if blk.fused is not None and self.fuse_shortcut else blk.conv3
        if (self.bneck and t1 is None and (blk.down is None or conv3 is blk.fused)
                and C.bneck_ok(x, blk.conv1, blk.conv2, conv3)):
            out = self._buf(tag + ("xa" if bi % 2 == 0 else "xb"), (B, H, W, conv3.cout))[sl]
            return C.bneck_fused(x, blk.conv1, blk.conv2, conv3, out=out, grid=_BN_GRID), None
        if t1 is None:
            t1 = C.conv2d(x, blk.conv1, out=self._buf(tag + "t1", (B, H, W, blk.conv1.cout))[sl])
        Ho, Wo = blk.conv2.out_hw(H, W)
        key = "xa" if bi % 2 == 0 else "xb"
        nxt = self.blocks[bi + 1] if bi + 1 < len(self.blocks) else None
        if (self.exp3 and blk.down is None and C.conv_exp_ok(blk.conv2, blk.conv3, t1, x)
                and not (chain and self.chain and nxt is not None and C.chain_ok(blk.conv3, nxt.conv1))):
            out = self._buf(tag + key, (B, Ho, Wo, blk.conv3.cout))[sl]
            if out.is_contiguous():
                return C.conv3x3_exp(t1, blk.conv2, blk.conv3, x, out=out), None
        t2 = C.conv2d(t1, blk.conv2, out=self._buf(tag + "t2", (B, Ho, Wo, blk.conv2.cout))[sl])
        out = self._buf(tag + key, (B, Ho, Wo, blk.conv3.cout))[sl]
        if blk.fused is not None and self.fuse_shortcut:
            if (chain and self.chain and nxt is not None and C.chain_dual_ok(blk.fused, nxt.conv1)
                    and (ch * Ho * Wo) % 64 == 0 and x.is_contiguous() and (H, W) == (Ho, Wo)):
                t1n = self._buf(tag + "t1", (B, Ho, Wo, nxt.conv1.cout))[sl]
                C.conv_chain(t2, blk.fused, None, out, nxt.conv1, t1n, x2=x)
                return out, t1n
            return C.conv2d(t2, blk.fused, x2=x, out=out), None
        if blk.down is not None:
            idn = C.conv2d(x, blk.down, out=self._buf(tag + "ds", (B, Ho, Wo, blk.down.cout))[sl])
            return C.conv2d(t2, blk.conv3, residual=idn, out=out), None
        if (chain and self.chain and nxt is not None and C.chain_ok(blk.conv3, nxt.conv1)
                and (ch * Ho * Wo) % 64 == 0 and x.is_contiguous()):
            t1n = self._buf(tag + "t1", (B, Ho, Wo, nxt.conv1.cout))[sl]
            C.conv_chain(t2, blk.conv3, x, out, nxt.conv1, t1n)
            return out, t1n
        return C.conv2d(t2, blk.conv3, residual=x, out=out), None

    def _lanes(self, n: int) -> list:
        lanes = getattr(self, "_lane_streams", None)
        if lanes is None or len(lanes) < n:
            lanes = self._lane_streams = [torch.cuda.Stream(self.device) for _ in range(n)]
        return lanes[:n]

    def logits_lanes(self, x: torch.Tensor, lanes: int, frames: bool = False,
                     stagger: int | None = None) -> torch.Tensor:
        """Forward split into ``lanes`` batch slices, each on its own HIP stream with its own
        workspace, forked from and joined back into the current stream.  Captured in one
        hipGraph the slices are independent branches: one slice's kernels fill the tail
        and launch gaps of the other's, which a single in-order chain leaves idle.  With
        ``stagger`` = block index, lane i+1 starts only once lane i has passed that block, so
        the memory-bound early stages of one lane overlap the compute-bound late stages of
        the other."""
        B = x.shape[0]
        if lanes <= 1 or B % lanes:
            return self.logits(x) if frames else self.logits_from_stem(x)
        out = self._buf("logits", (B, self.num_classes))
        cur = torch.cuda.current_stream(self.device)
        step = B // lanes
        gate = None
        for i, s in enumerate(self._lanes(lanes)):
            s.wait_stream(cur)
            if gate is not None:
                s.wait_event(gate)
            with torch.cuda.stream(s):
                xi = x[i * step:(i + 1) * step]
                tag = f"l{i}."
                hook = None
                if stagger is not None and i + 1 < lanes:
                    gate = torch.cuda.Event()
                    hook = (stagger, lambda ev=gate, st=s: ev.record(st))
                f = self.features_from_frames(xi, tag, after_block=hook) if frames \
                    else self.features_from_stem(xi, tag, after_block=hook)
                C.linear(f, self.fc, out=out[i * step:(i + 1) * step], work=self._fc_work(tag, f.shape[0]))
        for s in self._lanes(lanes):
            cur.wait_stream(s)
        return out

    # ---- two-part forward (frame-lane phase gating, elements/gpu/vision.py) -----------------
    SPLIT_BLOCK = 6          # end of stage 2: stem + stages 1-2 (memory-bound) | stages 3-4 (compute-bound)

    def logits_part_a(self, frames: torch.Tensor, tag: str = "") -> torch.Tensor:
        """uint8 frames -> activation after bottleneck ``SPLIT_BLOCK`` (a workspace buffer)."""
        B = frames.shape[0]
        S = self.image_size
        Ho, Wo = C.stem_out_hw(S, S)
        Hm, Wm = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
        pool = self._buf(tag + "pool", (B, Hm, Wm, 64))
        u8 = self._stem_u8_ok(frames)
        x = frames if frames.dtype != torch.uint8 or u8 else self.preprocess(frames, tag)
        if u8:
            x = C.stem_pool_u8(frames, self.stem, V.IMAGENET_MEAN, V.IMAGENET_STD, out=pool)
        elif self.fuse_stem_pool:
            x = C.stem_pool(x, self.stem, (S, S), out=pool)
        else:
            st = self._buf(tag + "stem", (B, Ho, Wo, 64))
            x = V.maxpool2d(C.conv2d(x, self.stem, out=st, image_hw=(S, S)), 3, 2, 1, out=pool)
        t1 = None
        for bi in range(self.SPLIT_BLOCK + 1):
            x, t1 = self._block(bi, x, tag, B, 0, B, t1, chain=bi < self.SPLIT_BLOCK)
        assert t1 is None, "the split must not cut a chained block boundary"
        return x

    def logits_part_b(self, x: torch.Tensor, tag: str = "") -> torch.Tensor:
        """Activation after bottleneck ``SPLIT_BLOCK`` -> logits."""
        B = x.shape[0]
        t1 = None
        for bi in range(self.SPLIT_BLOCK + 1, len(self.blocks)):
            x, t1 = self._block(bi, x, tag, B, 0, B, t1)
        f = V.avgpool(x, out=self._buf(tag + "gap", (B, x.shape[3])))
        return C.linear(f, self.fc, out=self._buf(tag + "logits", (B, self.num_classes)), work=self._fc_work(tag, B))

    def features(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 [B, H, W, 3] -> pooled features bf16 [B, 2048]."""
        return self.features_from_frames(frames)

    def logits_from_stem(self, x: torch.Tensor, tag: str = "") -> torch.Tensor:
        f = self.features_from_stem(x, tag)
        return C.linear(f, self.fc, out=self._buf(tag + "logits", (f.shape[0], self.num_classes)),
                        work=self._fc_work(tag, f.shape[0]))

    def topk_from_logits(self, lg: torch.Tensor):
        B = lg.shape[0]
        return V.softmax_topk(lg, self.topk,
                              prob=self._buf("prob", (B, self.topk), torch.float32),
                              index=self._buf("index", (B, self.topk), torch.int32))

    def logits(self, frames: torch.Tensor, tag: str = "") -> torch.Tensor:
        f = self.features_from_frames(frames, tag)
        return C.linear(f, self.fc, out=self._buf(tag + "logits", (f.shape[0], self.num_classes)),
                        work=self._fc_work(tag, f.shape[0]))

    def forward(self, frames: torch.Tensor):
        lg = self.logits(frames)
        B = lg.shape[0]
        return V.softmax_topk(lg, self.topk,
                              prob=self._buf("prob", (B, self.topk), torch.float32),
                              index=self._buf("index", (B, self.topk), torch.int32))

    __call__ = forward

    # ---- bookkeeping ----------------------------------------------------------------------
    def conv_specs(self):
        yield "stem", self.stem
        for i, b in enumerate(self.blocks):
            yield f"b{i}.conv1", b.conv1
            yield f"b{i}.conv2", b.conv2
            yield f"b{i}.conv3", b.conv3
            if b.down is not None:
                yield f"b{i}.down", b.down
        yield "fc", self.fc

    def flops_per_image(self) -> int:
        """Multiply-adds x 2 of every conv/FC at the configured resolution (≈ 8.2 GFLOP)."""
        total = 0
        S = self.image_size
        H, W = C.stem_out_hw(S, S)
        total += 2 * H * W * 64 * 3 * 49
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        for b in self.blocks:
            total += b.conv1.flops(1, H, W)
            Ho, Wo = b.conv2.out_hw(H, W)
            total += b.conv2.flops(1, H, W)
            total += b.conv3.flops(1, Ho, Wo)
            if b.down is not None:
                total += b.down.flops(1, H, W)
            H, W = Ho, Wo
        total += 2 * 2048 * self.num_classes
        return total

    def named_layers(self):
        return self.conv_specs()

    def config(self) -> dict:
        return {"num_classes": self.num_classes, "image_size": self.image_size, "topk": self.topk}

    def _weights_loaded(self):
        """Re-derive the K-concatenated conv3 + shortcut specs and the fused stem's LDS weight
        image from the loaded layers, in place (a captured hipGraph never re-enters Python, so
        the image must be refreshed here, not lazily at the next eager call)."""
        if getattr(self.stem, "_stem_pool_w", None) is not None:
            C.stem_pool_weight(self.stem)
        u8 = getattr(self.stem, "_stem_pool_u8_w", None)
        if u8 is not None:                          # the uint8 stem's 1/(255 std)-scaled image
            C.stem_pool_u8_weight(self.stem, u8[0][2])
        for b in self.blocks:
            if b.fused is None:
                continue
            k1 = b.conv3.weight.shape[1]
            b.fused.weight[:, :k1].copy_(b.conv3.weight)
            b.fused.weight[:, k1:].copy_(b.down.weight)
            if b.fused.bias is not None:
                b.fused.bias.copy_((b.conv3.bias if b.conv3.bias is not None else 0)
                                   + (b.down.bias if b.down.bias is not None else 0))

    # ---- fp32 torch reference (tests only) -------------------------------------------------
    def reference_logits(self, frames: torch.Tensor) -> torch.Tensor:
        from ..ops import reference as R
        x = R.preprocess_ref(frames, (self.image_size, self.image_size))
        x = R.conv_ref(x, self.stem)
        x = torch.nn.functional.max_pool2d(x, 3, 2, 1)
        for b in self.blocks:
            t = R.conv_ref(x, b.conv1)
            t = R.conv_ref(t, b.conv2)
            idn = R.conv_ref(x, b.down) if b.down is not None else x
            x = R.conv_ref(t, b.conv3, residual_nchw=idn)
        x = x.mean(dim=(2, 3))
        return R.linear_ref(x, self.fc)
