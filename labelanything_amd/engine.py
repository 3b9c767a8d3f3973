"""LamEngine: composes the libla_hip.so kernels into the LabelAnything inference path.

Data layout in HBM (all device-resident, reused across calls through a shape-keyed arena):
  * activations are row-major [pixels | tokens, channels] (NHWC); the fp32 residual stream is kept in fp32,
    every GEMM operand is a 16-bit copy written by the producing kernel's epilogue;
  * weights are repacked once per (device, dtype): nn.Linear layout [N, K] in 16 bit, conv weights flattened
    to the im2col column order, ConvTranspose2d(k2,s2) as [(ky,kx,cout), cin], q/k/v projections concatenated;
  * the SAM V operand is written pre-transposed ([b*heads, 64, Tpad]) by the qkv GEMM epilogue.

Each method cites the reference code it replaces (/root/reference/label_anything/...).
PyTorch is used for device memory, views/copies and the host-side prompt bookkeeping only.
"""
from __future__ import annotations


import dataclasses
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib as L
from .config import LamConfig, EncoderSpec, EncoderKind, encoder_kind
from .config import BlockNames, SAM_BLOCK, HF_BLOCK, DINOV2_BLOCK, DINOV3_BLOCK          # noqa: F401  (re-exported: train_encoder.py, tests)

Tensor = torch.Tensor


def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b * b


class Arena:
    """Shape-keyed cache of device buffers (no allocation in steady state; zero-filled buffers keep their padding)."""

    def __init__(self, device: torch.device):
        self.device = device
        self.bufs: Dict[tuple, Tensor] = {}

    def get(self, name: str, shape, dtype, zero: bool = False, init=None) -> Tensor:
        """init(t): called ONCE, when the buffer is created (constant contents that later launches never overwrite)."""
        key = (name, tuple(shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            try:
                t = (torch.zeros if zero else torch.empty)(tuple(shape), device=self.device, dtype=dtype)
            except RuntimeError as e:  # keep the substring the reference's OOM handler looks for (run.py:339-340)
                raise RuntimeError(f"HIP out of memory allocating {name}{tuple(shape)}: {e}") from e
            if init is not None:
                init(t)
            self.bufs[key] = t
        return t

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.bufs.values())


# Encoder GEMM groups that run in split precision (tools/error_budget.py): the 16-bit rounding of the WEIGHTS is
# the same perturbation for every token, so its effect survives attention and pooling instead of averaging out like the
# activation roundings, and the necks / patch embedding have no residual stream to dilute their error.
#   "qkv", "proj", "lin1", "lin2": weights as two 16-bit planes [W_hi | W_lo] (la_gemm a_kmod), activations 16-bit;
#   "v": only the V rows of the qkv weight carry the second plane (the qkv GEMM becomes a one-plane q/k launch and a two-plane V
#        launch).  tools/error_budget.py: rounding Wq / Wk perturbs the attention SCORES incoherently and washes out (cfg1 low-res
#        logits 9.5e-4 with only Wq, Wk split = the same as with no plane at all), the V projection is linear all the way to the
#        block output (7.0e-4 with only Wv split, 6.7e-4 with all three);
#   "patch", "neck": fp32-class products (fp16 plane pairs on both operands where the shape allows, exact-fp32 MFMA otherwise).
# Which groups are worth their cost was measured on the golden cases (profiles/r03_parity_groups.log) AND over other weight / episode
# seeds (tests/test_parity_seeds_gpu.py, profiles/r03_parity_seeds.log: the max-norm error moves by +-15 % with the seed; worst stage,
# tolerance 1e-3).  The 768+-wide encoders of the BASELINE configs keep patch / V / proj / neck - as second planes in round 2
# (6.6-8.0e-4 over the seeds tried; without proj 7.0-9.4e-4), as token-mean corrections since round 3 (5.6-8.0e-4); lin2's plane would
# buy another ~1e-4 for 8 % of the step.  Encoders narrower than 512 keep the full qkv, proj and lin2 planes (cheap there, and their
# share of the error is larger: sam_tiny 1.02e-3 -> 7.4e-4).
#   "vmean", "projmean": TOKEN-MEAN correction instead of a second plane (round 3).  With one plane token i errs by a_i . W_lo^T; what
#        survives attention and pooling is the part every token of an image shares, mean_i(a_i) . W_lo^T - a per-image vector.  It is
#        formed in fp32 from the token means of the GEMM operands (left behind by the LayerNorm / attention kernels that write them,
#        mean_fix) and ONE few-row exact-fp32 la_gemm per block against [Wo Wv_lo | Wo_lo], and carried as a pending per-image correction
#        R of the residual stream that every LayerNorm adds on the fly (la_layernorm_g).  V: softmax rows sum to one, so the vector
#        c_v = mean(x) Wv_lo^T that belongs on every V row of the image comes out of attention unchanged and goes through proj as
#        c_v Wo^T; proj adds mean(o) Wo_lo^T.  Emulated (tools/error_budget.py --mean) and measured: the same error as
#        the second planes for 3.5 ms instead of 8.7 ms of the cfg2 step.
PRECISE_FULL = ("patch", "qkv", "proj", "lin2", "neck")
PRECISE_WIDE = ("patch", "vmean", "projmean", "neck")
PRECISE_WIDE_PLANES = ("patch", "v", "proj", "neck")          # round 2's default: second weight planes for V and proj
PRECISE_DEFAULT = "auto"
PRECISE_GROUPS = ("patch", "qkv", "v", "proj", "lin1", "lin2", "neck", "vmean", "projmean")


def patch_kp(patch: int) -> int:
    """Columns of the patch-embedding operand: K = 3 p p when the patch side is a multiple of 8 (la_im2col_patch), else K rounded up to
    the multiple of 64 (at least 128) that la_im2col_patch_pad pads with zeros and every K % 64 == 0 path of la_gemm takes."""
    k = 3 * patch * patch
    return k if patch % 8 == 0 else max(128, -(-k // 64) * 64)


@dataclass(frozen=True)
class AttnGeo:
    """Geometry and form of one encoder block's attention, as LamEngine._attn_geo chose them."""
    pfx: str                      # arena buffers: pfx + ".qkv" + sfx, ".vt", ".ao"
    sfx: str
    bn: int                       # images
    rpg: int                      # tokens per image
    heads: int
    hdp: int
    scale: float
    g: int                        # side of the image's rel-pos grid; 0: plain attention
    ws: int                       # window side; 0: global
    nb: int                       # attention batches (images, or windows of all images)
    t: int                        # tokens per batch
    gg: int                       # grid side of a batch
    tpad: int                     # key slots per batch
    win16: bool
    form: str                     # "rows" (la_attn_fwd_rows) | "vt" (V^T epilogue) | "scatter" (V^T epilogue, window-order scatter) | "fp8"
    arows: int                    # rows of qkv and of the attention output
    o_chunks: int                 # 128-query blocks per image: column-sum partials of the attention output

    @property
    def ea(self) -> int:          # width of the q / k / v / attention-output blocks (== the stream's unless the heads are padded)
        return self.heads * self.hdp

    @property
    def nwy(self) -> int:
        return (self.g + self.ws - 1) // self.ws

    @property
    def parted(self) -> bool:     # qkv and the attention output are in window order
        return self.ws > 0 and self.form != "rows"


def rope_table(g: int, hd: int, theta: float) -> Tuple[Tensor, Tensor]:
    """(cos, sin), fp32 [g * g, hd] on the host: the rotary table of a g x g patch grid (transformers DINOv3ViTRopePositionEmbedding in
    eval mode, operation for operation).  Patch centres (i + 0.5) / g mapped to [-1, 1], row-major (y, x); inv_freq =
    theta^(-arange(0, 1, 4 / hd)); angles 2 pi coord (x) inv_freq flattened (y block, then x block) to hd / 2 and tiled twice."""
    if hd % 4:
        raise ValueError(f"rope_table: head width {hd} must be a multiple of 4")
    c = torch.arange(0.5, g, dtype=torch.float32) / g
    coords = 2.0 * torch.stack(torch.meshgrid(c, c, indexing="ij"), dim=-1).flatten(0, 1) - 1.0          # [g g, 2] = (y, x)
    inv_freq = 1 / theta ** torch.arange(0, 1, 4 / hd, dtype=torch.float32)                                # [hd / 4]
    angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2).tile(2)           # [g g, hd]
    return torch.cos(angles).contiguous(), torch.sin(angles).contiguous()


_BICUBIC: Dict[tuple, Tensor] = {}


def bicubic_matrix_t(gin: int, gout: int, device) -> Tensor:
    """B^T [gin^2, gout^2] of the linear map ``F.interpolate(x, (gout, gout), mode='bicubic', align_corners=False)`` on a gin x gin
    grid (transformers ViTEmbeddings.interpolate_pos_encoding under build_encoder.py:83-100), built once per geometry by pushing
    the identity through torch's own CPU kernel - the resample of the position table then is one small exact-fp32 product (and its
    backward the transposed one) instead of torch's device kernels (30 ms per step in the trainable-encoder step, most of it the
    atomics of upsample_bicubic2d_backward)."""
    key = (gin, gout, str(device))
    m = _BICUBIC.get(key)
    if m is None:
        eye = torch.eye(gin * gin).view(gin * gin, 1, gin, gin)
        m = F.interpolate(eye, size=(gout, gout), mode="bicubic", align_corners=False).reshape(gin * gin, gout * gout).contiguous().to(device)
        _BICUBIC[key] = m
    return m


def resolve_precise(cfg: LamConfig, precise, dtype: torch.dtype = torch.float16) -> tuple:
    """'auto' -> the measured default for this encoder width and operand type; None / () -> no split precision; else the given
    groups.  bf16 operands (8 mantissa bits) always take the full set: its activations alone cost more than fp16's weights."""
    if isinstance(precise, str):
        if precise != "auto":
            raise ValueError("precise must be 'auto', None or a sequence of group names")
        spec = cfg.encoder_spec
        wide = spec is not None and spec.dim >= 512 and dtype == torch.float16
        return PRECISE_WIDE if wide else PRECISE_FULL
    return tuple(precise or ())


class LamEngine:
    def __init__(self, cfg: LamConfig, weights: Dict[str, Tensor], device: torch.device, dtype: torch.dtype = torch.float16,
                 decoder_dtype: Optional[torch.dtype] = torch.float32, precise=PRECISE_DEFAULT, fuse_twoway: bool = True,
                 scope: str = "all", fuse_oneway: bool = True):
        """dtype: MFMA operand type of the image encoder and necks (>99% of the FLOPs).  decoder_dtype: operand type of the
        prompt encoder / mask decoder GEMMs - fp32 by default (exact-fp32 MFMA; ~1% of the FLOPs but the stage where
        16-bit operand rounding would dominate the logit error), or None to follow ``dtype``.  precise: encoder GEMM groups
        that run in split precision (see PRECISE_DEFAULT); () = every encoder GEMM with plain 16-bit operands.
        fuse_twoway: explicit constructor switch for A/B measurements (tools/) of the fused two-way kernels; the product never reads the
        environment.  fuse_oneway: the same for the OneWayTransformer of the mask decoder (la_twoway_i2t + la_stream_mlp per layer; False
        keeps the GEMM + attention + norm chain).  scope="encoder": only the image encoder's weights
        are packed (the trainer-private engine of train_encoder.HfEncoderGraph, re-packed after every optimizer step by
        ``repack_encoder``)."""
        if scope not in ("all", "encoder"):
            raise ValueError("scope must be 'all' or 'encoder'")
        self.scope = scope
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("compute dtype must be torch.float16 or torch.bfloat16")
        self.precise = frozenset(resolve_precise(cfg, precise, dtype))
        # opt-in (Lam.attn_fp8): QK^T of the plain (HF) attention on the fp8 MFMA - BASELINE configs[4].  3 mantissa bits on q and k cost
        # 1e-2-class logit error (profiles/r03_attn_fp8.log): never the parity configuration
        self.attn_fp8 = False
        self.patch_split = False                 # set by _patch_weight
        # decoder_dtype "f16x2": the IMAGE-side GEMM operands of the prompt encoder / mask decoder (the (P, hw, D) stream) are pairs
        # of fp16 planes [hi | lo] and their weights [W_hi | W_hi | W_lo] (LA_F16X2, la_hip.h): 3 fast-MFMA products instead of the
        # exact-fp32 MFMA, same accuracy class; the few-row token side stays exact fp32.
        self.isplit = isinstance(decoder_dtype, str) and decoder_dtype == "f16x2"
        if isinstance(decoder_dtype, str):
            if not self.isplit:
                raise ValueError("decoder_dtype must be a torch dtype, None or 'f16x2'")
            decoder_dtype = torch.float32
            # the narrowest image-side GEMM (output_upscaling.3, K = D / 4) needs 2 K % 64 == 0 for the plane-pair operand:
            # narrower decoders (test geometries) run the exact-fp32 MFMA throughout
            self.isplit = cfg.embed_dim % 128 == 0
        if not self.precise <= set(PRECISE_GROUPS):
            raise ValueError(f"unknown precise groups {sorted(self.precise - set(PRECISE_GROUPS))}; known: {PRECISE_GROUPS}")
        self.kmod: Dict[str, int] = {}      # packed-weight key -> a_kmod of its GEMM (split-precision planes)
        self.mean_kx: Dict[str, int] = {}   # block prefix -> columns of its '.mean.w32' that multiply mean(x) (the rest multiply mean(o))
        # the image side of the two-way transformers runs in the fused kernels (one read / one read + write of the stream per
        # attention, csrc/twoway.hip) for the published decoder geometry; fuse_twoway=False keeps the GEMM + attention + norm chain
        self.fuse_twoway = bool(fuse_twoway) and cfg.embed_dim in (256, 512) and cfg.dec_heads == 8 and decoder_dtype == torch.float32
        # fusion_transformer = "OneWayTransformer": per layer la_twoway_i2t (with norm1) + la_stream_mlp (with norm2), where both take the shape
        self.fuse_oneway = bool(fuse_oneway) and self.fuse_twoway and cfg.one_way and L.stream_mlp_ok(cfg.embed_dim, cfg.dec_mlp)
        # attention without V^T copies / window buffers (la_attn_fwd_rows) wherever its forms cover the block: plain attention, the 64 x 64
        # rel-pos grid, 16-slot windows; False keeps the V^T epilogue + window scatter path (A/B, and what the other geometries still use)
        self.attn_rows = True
        self.last_block_path: Optional[str] = None      # "plain" | "fold": the block driver vit_encoder took last (tests assert it)
        self.win_fused_cs = True           # folded SAM stack: the window blocks' token means of the attention output from the attention epilogue's column sums
                                           # (on the matrix pipe since round 6; as the global blocks always did) instead of a la_colmean16 pass (A/B: False)
        self.conv_implicit = True          # the necks' 3 x 3 convolution as an implicit GEMM on zero-bordered plane-pair maps (A/B: False = im2col + GEMM)
        self.conv_split = True             # the mask decoder's 32-channel spatial convolutions on la_conv3x3_split (A/B: False = la_conv3x3_f32)
        # LayerNorm folded into its neighbour GEMMs (round 6; LaGemmEpilogue.nstat_out / nstat_in): the residual GEMMs (patch embedding, proj,
        # lin2) also write the 16-bit copy of the stream and the partial sums of every row, q | k | v and lin1 run on gamma-folded weights
        # and normalise the product in their epilogue - no LayerNorm pass over the stream (24 launches, 10.4 ms of a 131 ms cfg2 step).
        # Wide fp16 encoders with one-plane q | k | v and lin1 weights (the measured default of the BASELINE encoders); emulated on the
        # fixtures before it was built (tools/error_budget.py --fold, profiles/r06_normfold_emulation.log).  False keeps the LayerNorm kernels.
        spec = cfg.encoder_spec
        self.norm_fold = (scope == "all" and spec is not None and dtype == torch.float16 and spec.dim >= 512 and spec.dim % 256 == 0
                          and spec.mlp % 256 == 0 and (3 * spec.heads * 64 * ((spec.head_dim + 63) // 64)) % 256 == 0
                          and not (self.precise & {"qkv", "v", "lin1"}))
        self.norm_fold_packed = self.norm_fold      # (the folded weights exist; Lam.norm_fold = False switches back to the LayerNorm kernels)
        self.ddt = dtype if decoder_dtype is None else decoder_dtype
        self.ddti = L._DT[self.ddt]
        L.lib()  # fail loudly if the HIP extension is missing
        self.cfg = cfg
        self.dev = device
        self.dt = dtype
        self.dti = L._DT[dtype]
        self.arena = Arena(device)
        self.w32: Dict[str, Tensor] = {k: v.detach().to(device=device, dtype=torch.float32).contiguous() for k, v in weights.items()}
        self.p: Dict[str, Tensor] = {}
        self._pe_cache: Dict[int, Tensor] = {}
        self._pe_tables: Dict[tuple, Tensor] = {}
        self._hfpos_cache: Dict[int, Tensor] = {}
        self._rope_cache: Dict[int, Tuple[Tensor, Tensor]] = {}
        self._pack()

    # ------------------------------------------------------------------------------------------------
    # weight packing (one-time layout transforms)
    # ------------------------------------------------------------------------------------------------
    def _h(self, t: Tensor) -> Tensor:
        return t.to(self.dt).contiguous()

    def _hd(self, t: Tensor) -> Tensor:
        return t.to(self.ddt).contiguous()

    @staticmethod
    def _split3(t: Tensor) -> Tensor:
        """[N, K] fp32 -> [N, 3K] fp16 = [W_hi | W_hi | W_lo] (pairs with A = [A_hi | A_lo], a_kmod = 2K)."""
        hi = t.to(torch.float16)
        lo = (t - hi.float()).to(torch.float16)
        return torch.cat([hi, hi, lo], dim=1).contiguous()

    def ibuf(self, name: str, rows: int, e: int) -> Tensor:
        """Image-side GEMM operand buffer: [rows, 2e] fp16 plane pairs in split mode, else a decoder-dtype [rows, e] buffer."""
        if self.isplit:
            return self.arena.get(name, (rows, 2 * e), torch.float16, False)
        return self.dbuf(name, (rows, e))

    @property
    def idti(self) -> int:
        return L.LA_F16X2 if self.isplit else self.ddti

    def igemm(self, a: Tensor, wkey: str, **kw) -> None:
        """GEMM with an image-side A operand against decoder weight ``wkey`` (split-plane aware)."""
        if self.isplit:
            w = self.p[wkey + "s"]
            L.gemm(a, w, a_kmod=2 * (w.shape[1] // 3), **kw)
        else:
            L.gemm(a, self.p[wkey], **kw)

    def _hw(self, key: str, t: Tensor, group: str) -> None:
        """Pack an encoder GEMM weight [N, K]: one 16-bit plane, or [W_hi | W_lo] when its group is precise."""
        t = t.contiguous()
        if group in self.precise and t.shape[1] % 64 == 0:
            hi = t.to(self.dt)
            lo = (t - hi.float()).to(self.dt)
            self.p[key] = torch.cat([hi, lo], dim=1).contiguous()
            self.kmod[key] = t.shape[1]
        else:
            self.p[key] = t.to(self.dt)
            self.kmod.pop(key, None)

    def _pack_fold(self, key: str, wt: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor) -> None:
        """The consumer side of a folded LayerNorm (LaGemmEpilogue.nstat_in): weight rn16(W diag(gamma)) as ``key + "n"``, its row sums
        (what multiplies the row mean) as ``.cn`` and b + W beta as ``.bn`` beside the plain packing of the same layer."""
        wf = (wt * gamma[None, :]).to(self.dt).contiguous()
        self.p[key + "n"] = wf
        self.p[key[:-2] + ".cn"] = wf.double().sum(1).float().contiguous()
        self.p[key[:-2] + ".bn"] = (bias.double() + wt.double() @ beta.double()).float().contiguous()

    def _pack_mean(self, pre: str, wv: Tensor, wo: Tensor, gamma: Tensor) -> None:
        """fp32 operand of the token-mean corrections of one block: rvec += [mean(x) | mean(o)] . [Wo Wv_lo | Wo_lo]^T, where *_lo is what
        the 16-bit plane of a weight lost (c_v = mean(x) Wv_lo^T belongs on every V row of the image, softmax rows sum to one, so it
        leaves attention unchanged and goes through proj as c_v Wo^T: one [E, E] product formed here, once)."""
        def cols(wv):
            c = []
            if "vmean" in self.precise:
                c.append((wo.double() @ (wv - wv.to(self.dt).float()).double()).float())      # [E, ea] . [ea, E]
            if "projmean" in self.precise:
                c.append((wo - wo.to(self.dt).float()).float())                                # [E, ea]
            return c

        if self.norm_fold and self.mean_planes:
            # the folded form multiplies the token means of the normalised rows BEFORE gamma: the lost plane is that of Wv diag(gamma)
            self.p[pre + ".mean.w32n"] = torch.cat(cols(wv * gamma[None, :]), dim=1).contiguous()
        if self.mean_planes:
            c = cols(wv)
            self.p[pre + ".mean.w32"] = torch.cat(c, dim=1).contiguous()
            self.mean_kx[pre] = c[0].shape[1] if "vmean" in self.precise else 0

    @property
    def mean_planes(self) -> bool:
        return "vmean" in self.precise or "projmean" in self.precise

    def mean_parts(self, at: AttnGeo, e: int):
        """Scratch of one block's fused column sums: (LayerNorm partials or None, attention partials or None) - see mean_fix."""
        xp = self.f32("mean.xpart", (at.bn * L.ln_cs_chunks(at.rpg) * e,)) if "vmean" in self.precise else None
        op = self.f32("mean.opart", (at.bn * max(at.o_chunks, _ceil(at.rpg, 128) // 128) * at.ea,)) if "projmean" in self.precise else None
        return xp, op

    def _mean_bar(self, pre: str, wm: Tensor, at: AttnGeo, e: int, xpart, x_chunks: int, opart, o_chunks: int, ao: Tensor) -> Tensor:
        """[mean(x) | mean(o)] per image, the left operand of a block's token-mean correction against wm.  xpart: column sums of the 16-bit
        qkv operand in x_chunks chunks per image, left by the kernel that wrote it; opart: column sums of the attention output per 128-query
        block (o_chunks per image), left by the attention kernel - or, o_chunks == 0, scratch for a separate pass over ao (la_colmean16,
        which undoes the window order of ao).  Chunks are folded in a fixed order: an image's vectors do not depend on the rest of the batch."""
        bn, rpg, kx = at.bn, at.rpg, self.mean_kx[pre]
        bar = self.f32("mean.bar", (bn, wm.shape[1]))
        if xpart is not None:
            L.colsum_fold(xpart, bn, x_chunks, e, 1.0 / rpg, bar[:, :kx])
        if opart is not None and o_chunks > 0:
            L.colsum_fold(opart, bn, o_chunks, at.ea, 1.0 / rpg, bar[:, kx:])
        elif opart is not None:
            obar = self.f32("mean.obar", (bn, at.ea))
            ws, g = (at.ws, at.g) if at.parted else (0, 0)
            L.colmean16(ao, bn, rpg, obar, opart, ws, g, g)
            bar[:, kx:].copy_(obar)
        return bar

    def mean_fix(self, pre: str, at: AttnGeo, e: int, xpart, opart, o_chunks: int, ao: Tensor, rvec: Tensor) -> None:
        """rvec[img] += mean(x) (Wo Wv_lo)^T + mean(o) Wo_lo^T for one attention block (see PRECISE_WIDE); xpart from the LayerNorm that
        wrote the qkv operand (la_layernorm_g), the rest as in _mean_bar."""
        wm = self.p[pre + ".mean.w32"]
        L.gemm(self._mean_bar(pre, wm, at, e, xpart, L.ln_cs_chunks(at.rpg), opart, o_chunks, ao), wm, res=rvec, out32=rvec)

    def _fold_mean(self, pre: str, at: AttnGeo, e: int, xpart, opart, o_chunks: int, ao: Tensor) -> Optional[Tensor]:
        """The block's token-mean correction as a FRESH per-image vector (the proj GEMM's epilogue adds it to the stream: nothing stays
        pending): dR[img] = [mean(z) | mean(o)] . [Wo (Wv gamma)_lo | Wo_lo]^T, z = the normalised rows before gamma (la_norm_finalize)."""
        if not self.mean_planes:
            return None
        wm = self.p[pre + ".mean.w32n"]
        dr = self.f32("mean.dr", (at.bn, e))
        L.gemm(self._mean_bar(pre, wm, at, e, xpart, L.norm_cs_chunks(at.rpg), opart, o_chunks, ao), wm, out32=dr)
        return dr

    def _hw_qkv(self, key: str, t: Tensor, bias: Tensor, ea: int) -> None:
        """Pack a fused qkv weight [3 ea, K] + bias.  Group "qkv": planes for all rows; group "v": a one-plane [2 ea, K] q/k weight and
        a two-plane [ea, 2 K] V weight (two launches, qkv_gemm); else one plane."""
        self.p[key[:-2] + ".b"] = bias
        # q | k | v of a token whose LayerNorm output was zero-padded (pad-after-norm windows, image_encoder.py:160-172): the bias, as the
        # GEMM's 16-bit epilogue would round it - the row la_attn_fwd_rows reads for window tokens beyond the image
        self.p[key[:-2] + ".pad16"] = bias.to(self.dt).contiguous()
        if "qkv" not in self.precise and "v" in self.precise and t.shape[1] % 64 == 0 and (2 * ea) % 8 == 0:
            self.p[key + ".qk"] = t[: 2 * ea].to(self.dt).contiguous()
            self._hw(key + ".v", t[2 * ea:], "v")
            self.p.pop(key, None)
            return
        self._hw(key, t, "qkv")

    def qkv_gemm(self, x: Tensor, key: str, qkv: Tensor, vt: Tensor, ea: int, rowmap=None, **vtkw) -> None:
        """qkv[:, :2 ea] = q, k rows of x W^T + b; V goes transposed to vt (la_gemm vt epilogue) - one launch, or two when only the V
        rows of the weight carry a second plane.  rowmap = (map, p): output row map of both (image-order tokens -> window order)."""
        b = self.p[key[:-2] + ".b"]
        mkw = {} if rowmap is None else {"map": rowmap[0], "p": rowmap[1]}
        # vt None: no V^T copy (la_attn_fwd_rows reads the v columns), every column through the plain row-major epilogue
        if (key + ".qk") in self.p:
            vkw = {} if vt is None else dict(vt=vt, vt_col0=0, **vtkw)
            L.gemm(x, self.p[key + ".qk"], bias=b[: 2 * ea], out16=qkv[:, : 2 * ea], **mkw)
            L.gemm(x, self.p[key + ".v"], bias=b[2 * ea:], out16=qkv[:, 2 * ea:], a_kmod=self.kmod.get(key + ".v", 0), **vkw, **mkw)
        else:
            vkw = {} if vt is None else dict(vt=vt, vt_col0=2 * ea, **vtkw)
            self.gemm_w(x, key, bias=b, out16=qkv, **vkw, **mkw)

    def _patch_weight(self, pw: Tensor) -> Tensor:
        """Patch-embed weight [dim, 3 p p]: plain 16-bit; or, in the split-precision group "patch", fp16 plane triples
        [W_hi | W_hi | W_lo] against [A_hi | A_lo] patches (three fp16 MFMA products, ~21 mantissa bits; 2.8x the rate of
        the exact-fp32 MFMA it replaces) - fp32 for bf16 operands, whose planes would carry 16 bits only.  A patch side that is no multiple
        of 8 (DINOv2's 14: K = 588) gets zero columns up to ``patch_kp`` first, in fp32, which la_im2col_patch_pad's zero columns meet."""
        kp = patch_kp(math.isqrt(pw.shape[1] // 3))
        if kp != pw.shape[1]:
            pw = F.pad(pw, (0, kp - pw.shape[1]))
        if "patch" not in self.precise:
            return self._h(pw)
        self.patch_split = self.dt == torch.float16 and pw.shape[1] % 64 == 0
        return self._split3(pw) if self.patch_split else pw.contiguous()

    def patches(self, name: str, images: Tensor, rows: int, patch: int):
        """im2col of the patch embedding in the operand form _patch_weight chose; returns (A, extra la_gemm keywords)."""
        k = patch_kp(patch)

        def gather(a: Tensor, split: bool = False) -> None:
            if patch % 8:
                L.im2col_patch_pad(images, patch, k, a, split=split)
            else:
                L.im2col_patch(images, patch, a, split=split)

        if "patch" not in self.precise:
            a = self.buf(name, (rows, k))
            gather(a)
            return a, {}
        if self.patch_split:
            a = self.buf(name, (rows, 2 * k), torch.float16)
            gather(a, split=True)
            return a, {"a_kmod": 2 * k}
        a = self.buf(name, (rows, k), torch.float32)
        gather(a)
        return a, {}

    def gemm_w(self, a: Tensor, key: str, **kw) -> None:
        """la_gemm against the packed encoder weight ``key`` (split-precision aware)."""
        L.gemm(a, self.p[key], a_kmod=self.kmod.get(key, 0), **kw)

    @property
    def head_pad(self) -> int:
        """Encoder head width as the attention kernels see it: the next multiple of 64 (64 or 128).  Heads of another
        width (SAM ViT-H: 80) get zero weight rows / bias entries / table columns for the extra q, k, v dims and zero
        proj columns, which changes neither q.k nor the projected output."""
        hd = self.cfg.encoder_spec.head_dim
        hdp = 64 * ((hd + 63) // 64)
        if hdp > 128:
            raise NotImplementedError(f"encoder head_dim {hd} > 128 is not built")
        return hdp

    @staticmethod
    def _pad_heads_out(t: Tensor, groups: int, hd: int, hdp: int) -> Tensor:
        """[groups*hd, ...] -> [groups*hdp, ...]: zero rows appended to every head block of an output dimension."""
        if hd == hdp:
            return t.contiguous()
        v = t.reshape(groups, hd, *t.shape[1:])
        pad = torch.zeros(groups, hdp - hd, *t.shape[1:], dtype=t.dtype, device=t.device)
        return torch.cat([v, pad], dim=1).reshape(groups * hdp, *t.shape[1:]).contiguous()

    @staticmethod
    def _pad_heads_in(t: Tensor, groups: int, hd: int, hdp: int) -> Tensor:
        """[N, groups*hd] -> [N, groups*hdp]: zero columns appended to every head block of the input dimension."""
        if hd == hdp:
            return t.contiguous()
        v = t.reshape(t.shape[0], groups, hd)
        return F.pad(v, (0, hdp - hd)).reshape(t.shape[0], groups * hdp).contiguous()

    def _pack_attn(self, pre: str, fuse: str) -> None:
        """decoder Attention (common.py:57-148).  fuse: 'qkv' (same input), 'qk' (q,k share input), 'none'."""
        w, p = self.w32, self.p
        if fuse == "qkv":
            p[pre + ".qkv.w"] = self._hd(torch.cat([w[pre + ".q_proj.weight"], w[pre + ".k_proj.weight"], w[pre + ".v_proj.weight"]]))
            p[pre + ".qkv.b"] = torch.cat([w[pre + ".q_proj.bias"], w[pre + ".k_proj.bias"], w[pre + ".v_proj.bias"]]).contiguous()
        if fuse == "qk":
            p[pre + ".qk.w"] = self._hd(torch.cat([w[pre + ".q_proj.weight"], w[pre + ".k_proj.weight"]]))
            p[pre + ".qk.b"] = torch.cat([w[pre + ".q_proj.bias"], w[pre + ".k_proj.bias"]]).contiguous()
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            p[f"{pre}.{n}.w"] = self._hd(w[f"{pre}.{n}.weight"])
            if self.isplit:
                p[f"{pre}.{n}.ws"] = self._split3(w[f"{pre}.{n}.weight"])
            if self.fuse_twoway and (".cross_attn_" in pre or pre.endswith("final_attn_token_to_image")):
                hi = w[f"{pre}.{n}.weight"].to(torch.float16).contiguous()       # fp16 plane pair of the fused kernels (csrc/twoway.hip)
                p[f"{pre}.{n}.planes"] = (hi, (w[f"{pre}.{n}.weight"] - hi.float()).to(torch.float16).contiguous())

    def _pack_mlp(self, pre: str) -> None:
        self.p[pre + ".lin1.w"] = self._hd(self.w32[pre + ".lin1.weight"])
        self.p[pre + ".lin2.w"] = self._hd(self.w32[pre + ".lin2.weight"])

    def _pack_two_way(self, pre: str) -> None:
        for l in range(2):
            lp = f"{pre}.layers.{l}"
            self._pack_attn(lp + ".self_attn", "qkv" if l == 0 else "qk")
            self._pack_attn(lp + ".cross_attn_token_to_image", "none")
            self._pack_attn(lp + ".cross_attn_image_to_token", "none")
            self._pack_mlp(lp + ".mlp")
        self._pack_attn(pre + ".final_attn_token_to_image", "none")

    def _pack_one_way(self, pre: str) -> None:
        """OneWayTransformer (transformer.py:26-154): per layer the image -> token attention and the stream MLP.  norm3 is never read."""
        w, p = self.w32, self.p
        for l in range(2):
            lp = f"{pre}.layers.{l}"
            self._pack_attn(lp + ".cross_attn_image_to_token", "none")
            self._pack_mlp(lp + ".mlp")
            for n in ("lin1", "lin2"):
                wt = w[f"{lp}.mlp.{n}.weight"]
                if self.isplit:
                    p[f"{lp}.mlp.{n}.ws"] = self._split3(wt)
                if self.fuse_oneway:                # fp16 plane pair of la_stream_mlp (csrc/stream_mlp.hip)
                    hi = wt.to(torch.float16).contiguous()
                    p[f"{lp}.mlp.{n}.planes"] = (hi, (wt - hi.float()).to(torch.float16).contiguous())

    def _pack_conv_neck(self, pre: str) -> None:
        w = self.w32
        cast = (lambda t: t.contiguous()) if "neck" in self.precise else self._h
        self.p[pre + ".0.w"] = cast(w[pre + ".0.weight"].flatten(1))
        w2 = w[pre + ".2.weight"].permute(0, 2, 3, 1).flatten(1)                            # [Cout, (ky,kx,cin)]
        self.p[pre + ".2.w"] = cast(w2)
        # fp16 operands: the 3x3 conv of the precise neck runs on plane pairs (LN -> [hi | lo] -> im2col -> three fp16 products, ~21
        # mantissa bits) instead of the exact-fp32 implicit GEMM: 2.5x faster in the same accuracy class
        if "neck" in self.precise and self.dt == torch.float16 and w2.shape[0] % 32 == 0 and w2.shape[1] % 32 == 0:
            self.p[pre + ".2.ws"] = self._split3(w2)
        # ... and so does the 1 x 1 conv when its input arrives as plane pairs (conv_neck xs: the SAM stack's last pass over the stream
        # writes them, la_add_rowvec_split): 393216 x 256 x 768 in 0.7 ms instead of 1.6 ms on the exact-fp32 MFMA
        w0 = w[pre + ".0.weight"].flatten(1)
        if "neck" in self.precise and self.dt == torch.float16 and w0.shape[1] % 64 == 0 and w0.shape[0] % 32 == 0:
            self.p[pre + ".0.ws"] = self._split3(w0)

    def _pack_block(self, bp: str, nm: BlockNames) -> None:
        """One encoder block's GEMM weights under the packed keys both kinds share: ``.qkv.w`` / ``.b`` / ``.pad16`` (q | k | v concatenated,
        heads zero-padded to head_pad), ``.proj.w``, ``.lin1.w``, ``.lin2.w``, the token-mean operands ``.mean.w32`` / ``.mean.w32n`` and, with
        norm_fold, the gamma-folded ``.qkv.wn`` / ``.bn`` / ``.cn`` and ``.lin1.wn`` / ``.bn`` / ``.cn``."""
        w, spec = self.w32, self.cfg.encoder_spec
        hd, hdp = spec.head_dim, self.head_pad
        ea = spec.heads * hdp
        qkv_w = self._pad_heads_out(torch.cat([w[f"{bp}.{n}.weight"] for n in nm.qkv]), 3 * spec.heads, hd, hdp)
        qkv_b = self._pad_heads_out(torch.cat([w[f"{bp}.{n}.bias"] for n in nm.qkv]), 3 * spec.heads, hd, hdp)
        proj_w = self._pad_heads_in(w[f"{bp}.{nm.proj}.weight"], spec.heads, hd, hdp)
        self._hw_qkv(bp + ".qkv.w", qkv_w, qkv_b, ea)
        self._hw(bp + ".proj.w", proj_w, "proj")
        self._pack_mean(bp, qkv_w[2 * ea:], proj_w, w[f"{bp}.{nm.norm1}.weight"])
        if self.norm_fold:
            self._pack_fold(bp + ".qkv.w", qkv_w, qkv_b, w[f"{bp}.{nm.norm1}.weight"], w[f"{bp}.{nm.norm1}.bias"])
            self._pack_fold(bp + ".lin1.w", w[f"{bp}.{nm.lin1}.weight"], w[f"{bp}.{nm.lin1}.bias"], w[f"{bp}.{nm.norm2}.weight"],
                            w[f"{bp}.{nm.norm2}.bias"])
        self._hw(bp + ".lin1.w", w[f"{bp}.{nm.lin1}.weight"], "lin1")
        self._hw(bp + ".lin2.w", w[f"{bp}.{nm.lin2}.weight"], "lin2")

    def _pack(self) -> None:
        cfg, w, p = self.cfg, self.w32, self.p
        spec = cfg.encoder_spec
        if spec is not None and spec.kind == "sam":
            pre = "image_encoder"
            pw = w[pre + ".patch_embed.proj.weight"].flatten(1)
            p[pre + ".patch.w"] = self._patch_weight(pw)
            p[pre + ".pos"] = w[pre + ".pos_embed"].reshape(-1, spec.dim).contiguous()
            g = spec.img_size // spec.patch
            hd, hdp = spec.head_dim, self.head_pad
            for i in range(spec.depth):
                bp = SAM_BLOCK.prefix.format(i)
                self._pack_block(bp, SAM_BLOCK)
                size = g if i in spec.global_idx else spec.window
                for ax in ("h", "w"):
                    tab = w[f"{bp}.attn.rel_pos_{ax}"]
                    if tab.shape[0] != 2 * size - 1:   # get_rel_pos linear resampling (image_encoder.py:321-330), constant per model
                        tab = F.interpolate(tab.t().unsqueeze(0), size=2 * size - 1, mode="linear")[0].t()
                    p[f"{bp}.tab{ax}"] = self._h(F.pad(tab, (0, hdp - hd)))
            self._pack_conv_neck(pre + ".neck")
        elif spec is not None:
            pre, kind, nm = "image_encoder", self.kind, self.block_names
            p[pre + ".patch.w"] = self._patch_weight(w[f"{pre}.{kind.patch}.weight"].flatten(1))
            if not kind.pos_table:          # (with a table the prefix row depends on the input's grid: _hf_pos)
                p[pre + ".prefix"] = torch.cat([w[f"{pre}.{n}"][0] for n in kind.prefix]).contiguous()
            for i in range(spec.depth):
                if kind.layer_scale:
                    self._fold_layer_scale(nm.prefix.format(i), nm)
                self._pack_block(nm.prefix.format(i), nm)
        if self.scope == "encoder":
            return
        if cfg.lam_neck:
            self._pack_conv_neck("neck")
        pe = "prompt_encoder"
        p[pe + ".type_emb"] = torch.cat([w[f"{pe}.point_embeddings.{i}.weight"] for i in range(4)]).contiguous()
        p[pe + ".mask_w"] = [w[pe + ".mask_downscaling.0.weight"].contiguous(), w[pe + ".mask_downscaling.0.bias"],
                             w[pe + ".mask_downscaling.1.weight"], w[pe + ".mask_downscaling.1.bias"],
                             w[pe + ".mask_downscaling.3.weight"].contiguous(), w[pe + ".mask_downscaling.3.bias"],
                             w[pe + ".mask_downscaling.4.weight"], w[pe + ".mask_downscaling.4.bias"],
                             w[pe + ".mask_downscaling.6.weight"].flatten(1).contiguous(), w[pe + ".mask_downscaling.6.bias"],
                             w[pe + ".not_a_mask_embed.weight"].flatten().contiguous(), w[pe + ".no_mask_embed.weight"].flatten().contiguous()]
        self._pack_two_way(pe + ".transformer")
        for blk in ("sparse_embedding_attention", "class_attention", "class_example_attention", "example_attention"):
            if f"{pe}.{blk}.norm.weight" in w:
                self._pack_attn(f"{pe}.{blk}.attn", "qkv")
                self._pack_mlp(f"{pe}.{blk}.mlp")
        if cfg.embedding_extraction == "cross_attention":
            self._pack_extraction(pe + ".embedding_extraction")
        md = "mask_decoder"
        if cfg.one_way:
            self._pack_one_way(md + ".transformer")
        else:
            self._pack_two_way(md + ".transformer")
        for i in range(3):
            p[f"{md}.class_mlp.{i}.w"] = self._hd(w[f"{md}.class_mlp.layers.{i}.weight"])
        # ConvTranspose2d weight (Cin, Cout, 2, 2) -> GEMM weight [(ky, kx, cout), cin]
        p[md + ".up0.w"] = self._hd(w[md + ".output_upscaling.0.weight"].permute(2, 3, 1, 0).flatten(0, 2))
        p[md + ".up3.w"] = self._hd(w[md + ".output_upscaling.3.weight"].permute(2, 3, 1, 0).flatten(0, 2))
        if self.isplit:
            p[md + ".up0.ws"] = self._split3(w[md + ".output_upscaling.0.weight"].permute(2, 3, 1, 0).flatten(0, 2))
            p[md + ".up3.ws"] = self._split3(w[md + ".output_upscaling.3.weight"].permute(2, 3, 1, 0).flatten(0, 2))
        if cfg.spatial_convs:
            for i in range(cfg.spatial_convs):
                p[f"{md}.sc{i}.w"] = self._hd(w[f"{md}.spatial_convs.{3 * i}.weight"].permute(0, 2, 3, 1).flatten(1))

    @property
    def kind(self) -> EncoderKind:
        return encoder_kind(self.cfg.encoder_spec.kind)

    @property
    def block_names(self) -> BlockNames:
        """Block names of the encoder's stack, with the LayerNorm eps of the spec where the kind takes it from there."""
        kind = self.kind
        return dataclasses.replace(kind.blocks, eps=self.cfg.encoder_spec.ln_eps) if kind.spec_eps else kind.blocks

    def _fold_layer_scale(self, bp: str, nm: BlockNames) -> None:
        """DINOv3ViTLayer / Dinov2Layer: x += lambda1 * o_proj(attn), x += lambda2 * down_proj(mlp).  The LayerScale vectors are folded, in
        fp32 and before the 16-bit packing, into the rows and the bias of the kind's two projections (EncoderKind.layer_scale), under the derived
        names ``nm.proj`` / ``nm.lin2``, so that the residual epilogues of the block drivers stay what they are; a key projection without
        a bias gets a zero one."""
        w = self.w32
        osrc, dsrc = self.kind.layer_scale
        for src, dst, ls in ((osrc, nm.proj, "layer_scale1"), (dsrc, nm.lin2, "layer_scale2")):
            if self.cfg.encoder_spec.layer_scale:
                lam = w[f"{bp}.{ls}.lambda1"]
                w[f"{bp}.{dst}.weight"] = (lam[:, None] * w[f"{bp}.{src}.weight"]).contiguous()
                w[f"{bp}.{dst}.bias"] = (lam * w[f"{bp}.{src}.bias"]).contiguous()
            else:
                w[f"{bp}.{dst}.weight"], w[f"{bp}.{dst}.bias"] = w[f"{bp}.{src}.weight"], w[f"{bp}.{src}.bias"]
        if not self.cfg.encoder_spec.key_bias:
            w[f"{bp}.{nm.qkv[1]}.bias"] = torch.zeros_like(w[f"{bp}.{nm.qkv[0]}.bias"])

    def _pack_extraction(self, ex: str) -> None:
        """EmbeddingTransformer (prompt_encoder.py:280-298).  The k / v projections stay fp32 matrices: la_extract_fold / la_extract_unfold
        apply them per head to the few query rows, the stream itself is never projected.  Layer 0's input is the learned queries, the same
        for every pair, so its folded queries are a constant of the weights: computed here, once."""
        w, p, cfg = self.w32, self.p, self.cfg
        d, n = cfg.embed_dim, int(cfg.embeddings_per_example)
        for l in range(2):
            lp = f"{ex}.layers.{l}"
            for nm in ("q_proj", "out_proj"):
                p[f"{lp}.cross_attn_image_to_token.{nm}.w"] = self._hd(w[f"{lp}.cross_attn_image_to_token.{nm}.weight"])
            self._pack_mlp(lp + ".mlp")
        ca = ex + ".layers.0.cross_attn_image_to_token"
        emb = w[ex + ".embeddings.weight"].contiguous()
        q0 = torch.empty(n, d // 2, device=self.dev, dtype=torch.float32)
        L.gemm(self._hd(emb), p[ca + ".q_proj.w"], bias=w[ca + ".q_proj.bias"], out32=q0)
        qt0 = torch.empty(L.EXTRACT_HEADS * n, d, device=self.dev, dtype=torch.float32)
        L.extract_fold(q0, w[ca + ".k_proj.weight"], 1, n, d, qt0)
        p[ex + ".qt0"] = qt0

    def repack_encoder(self, weights: Dict[str, Tensor]) -> None:
        """Refresh the packed image-encoder weights from ``weights`` (live parameters after an optimizer step); the arena, the cached
        positional tables that do not depend on parameters and everything outside the encoder stay.  Only for scope="encoder" engines."""
        if self.scope != "encoder":
            raise RuntimeError("repack_encoder is for scope='encoder' engines; full engines are rebuilt by Lam.engine()")
        for k, v in weights.items():
            if k.startswith("image_encoder."):
                self.w32[k] = v.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        self._hfpos_cache.clear()          # resampled position embeddings are functions of a parameter
        self._pack()

    # ------------------------------------------------------------------------------------------------
    # small helpers
    # ------------------------------------------------------------------------------------------------
    def h2d(self, t: Tensor, dtype=None) -> Tensor:
        """Small host tensor -> device without stalling the launch queue (pinned staging + async copy)."""
        if t.is_cuda:
            return t.to(self.dev, dtype) if dtype is not None else t.to(self.dev)
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous().pin_memory().to(self.dev, non_blocking=True)

    def buf(self, name, shape, dtype=None, zero=False, init=None) -> Tensor:
        return self.arena.get(name, shape, self.dt if dtype is None else dtype, zero, init)

    def dbuf(self, name, shape) -> Tensor:
        return self.arena.get(name, shape, self.ddt, False)

    def dln(self, x, name, eps, **kw):
        L.layernorm(x, self.w32[name + ".weight"], self.w32[name + ".bias"], eps, dt=self.ddti, **kw)

    def f32(self, name, shape, zero=False) -> Tensor:
        return self.arena.get(name, shape, torch.float32, zero)

    def dense_pe(self, g: int) -> Tensor:
        """[g*g, D] fp32, cached per grid (input independent; prompt_encoder.py:213-224)."""
        t = self._pe_cache.get(g)
        if t is None:
            t = torch.empty(g * g, self.cfg.embed_dim, device=self.dev, dtype=torch.float32)
            L.dense_pe(self.w32["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"], g, self.cfg.embed_dim, t)
            self._pe_cache[g] = t
        return t

    def ln(self, x, name, eps, rvec=None, rpg=0, **kw):
        """LayerNorm of x (+ the pending per-image corrections rvec[row // rpg] of the mean planes, never written back)."""
        if rvec is not None:       # (colsum_part=...: also leave the column sums of the stored rows, mean_fix)
            L.layernorm_g(x, rvec, rpg, self.w32[name + ".weight"], self.w32[name + ".bias"], eps, dt=self.dti, **kw)
        else:
            L.layernorm(x, self.w32[name + ".weight"], self.w32[name + ".bias"], eps, dt=self.dti, **kw)

    # ------------------------------------------------------------------------------------------------
    # conv neck: 1x1 conv -> LN2d -> 3x3 conv -> LN2d on NHWC rows (image_encoder.py:92-108, build_lam.py:150-171)
    # ------------------------------------------------------------------------------------------------
    def conv_neck(self, pre: str, x16: Optional[Tensor], bn: int, g: int, tag: str, x32: Optional[Tensor] = None,
                  xs: Optional[Tensor] = None) -> Tensor:
        """xs: x32 as fp16 plane pairs [rows, 2 Cin] (LA_F16X2), when the caller's last pass over the stream wrote them."""
        cout = self.p[pre + ".0.w"].shape[0]
        rows = bn * g * g
        a = self.f32(tag + ".n0", (rows, cout))
        if "neck" in self.precise:      # fp32-level products on the fp32 stream itself (no single 16-bit copy of the input at all)
            if xs is not None and (pre + ".0.ws") in self.p:
                L.gemm(xs, self.p[pre + ".0.ws"], out32=a, a_kmod=xs.shape[1])
            else:
                L.gemm(x32, self.p[pre + ".0.w"], out32=a)
            a1 = None
            if (pre + ".2.ws") not in self.p:
                a1 = self.f32(tag + ".n1f", (rows, cout))
                L.layernorm(a, self.w32[pre + ".1.weight"], self.w32[pre + ".1.bias"], 1e-6, out32=a1, dt=L.LA_F32)
            if (pre + ".2.ws") in self.p and self.conv_implicit and cout % 64 == 0 and cout % 256 == 0 and rows > 512:
                # IMPLICIT 3 x 3 convolution (round 6): the LayerNorm writes its plane pairs into the interior of zero-bordered
                # [bn, g + 2, g + 2] maps, the GEMM's k-tiles read the nine taps as wave-uniform shifts of its source base
                # (LA_MAP_CONV3X3) - no im2col buffer (18 x the map written and read again: 1.1 ms + most of the 1.2 ms GEMM's traffic) - and
                # the last LayerNorm gathers the interior rows.  Border rows of the product are computed and never read.
                gp = g + 2
                mp, guard = bn * gp * gp, gp + 1
                a1p = self.arena.get(tag + ".n1p", (mp + 2 * guard, 2 * cout), torch.float16, True)      # zero once: borders and guard rows stay zero
                L.layernorm(a, self.w32[pre + ".1.weight"], self.w32[pre + ".1.bias"], 1e-6, out16=a1p[guard:], dt=L.LA_F16X2, window=-1, H=g, W=g)
                a2p = self.f32(tag + ".n2p", (mp, cout))
                L.gemm(a1p[guard:guard + mp], self.p[pre + ".2.ws"], out32=a2p, amap=L.MAP_CONV3X3, p=(gp, cout, 2 * cout, 0, 0))
                out = self.f32(tag + ".out", (rows, cout))
                L.layernorm(a2p, self.w32[pre + ".3.weight"], self.w32[pre + ".3.bias"], 1e-6, out32=out, dt=L.LA_F32, window=-2, H=g, W=g)
                return out
            if (pre + ".2.ws") in self.p:
                a1s = self.buf(tag + ".n1s", (rows, 2 * cout), torch.float16)
                L.layernorm(a, self.w32[pre + ".1.weight"], self.w32[pre + ".1.bias"], 1e-6, out16=a1s, dt=L.LA_F16X2)
                col = self.buf(tag + ".cols", (rows, 18 * cout), torch.float16)
                L.im2col_3x3(a1s, bn, g, g, cout, col, split=True)
                L.gemm(col, self.p[pre + ".2.ws"], out32=a, a_kmod=18 * cout)
            elif cout % 32 == 0:
                L.conv3x3_f32(a1, bn, g, g, cout, self.p[pre + ".2.w"], None, cout, a)
            else:
                col = self.f32(tag + ".colf", (rows, 9 * cout))
                L.im2col_3x3(a1, bn, g, g, cout, col)
                L.gemm(col, self.p[pre + ".2.w"], out32=a)
            out = self.f32(tag + ".out", (rows, cout))
            L.layernorm(a, self.w32[pre + ".3.weight"], self.w32[pre + ".3.bias"], 1e-6, out32=out, dt=L.LA_F32)
            return out
        L.gemm(x16, self.p[pre + ".0.w"], out32=a)
        a16 = self.buf(tag + ".n1", (rows, cout))
        self.ln(a, pre + ".1", 1e-6, out16=a16)
        col = self.buf(tag + ".col", (rows, 9 * cout))
        L.im2col_3x3(a16, bn, g, g, cout, col)
        L.gemm(col, self.p[pre + ".2.w"], out32=a)
        out = self.f32(tag + ".out", (rows, cout))
        self.ln(a, pre + ".3", 1e-6, out32=out)
        return out

    # ------------------------------------------------------------------------------------------------
    # image encoders: one transformer block stack (plain or folded) behind a SAM ViTDet and a HuggingFace ViT entry / exit
    # ------------------------------------------------------------------------------------------------
    def _check_encoder_input(self, images: Tensor) -> None:
        spec: EncoderSpec = self.cfg.encoder_spec
        _ = self.head_pad          # raises for head widths beyond 128
        if images.shape[-1] % spec.patch or self.cfg.vit_patch_size != spec.patch:
            raise ValueError(f"image side {images.shape[-1]} / vit_patch_size {self.cfg.vit_patch_size} do not match the "
                             f"encoder's {spec.patch}x{spec.patch} patches")

    def _attn_geo(self, pfx: str, bn: int, rpg: int, g: int = 0, ws: int = 0) -> AttnGeo:
        """Geometry and form of the attention of one block over bn images of rpg tokens.  g: side of the image's rel-pos grid (SAM), 0 =
        plain attention (HF, CLS row included); ws: window side, 0 = a global block."""
        spec: EncoderSpec = self.cfg.encoder_spec
        hdp = self.head_pad
        if ws:
            nwy = (g + ws - 1) // ws
            nb, t, gg = bn * nwy * nwy, ws * ws, ws
        else:
            nb, t, gg = bn, rpg, g
        win16 = ws > 0 and gg <= 16      # windows: V^T / K in 16-wide padded slot order (LA_ATTN_RELPOS_WIN16)
        fp8 = not g and self.attn_fp8 and hdp == 64          # (the fp8 QK^T kernel keeps its V^T operand)
        # No V^T copy, no window buffers (la_attn_fwd_rows): the q | k | v GEMM of EVERY block walks the image-order tokens with its plain
        # row-major epilogue; attention stages V tiles row-major (LDS transpose reads) and, for 14 x 14 windows, addresses the image's
        # tokens directly (tokens beyond the image are the bias row); its output is in image order, so proj is a plain GEMM as well.
        # Measured (profiles/r05_notes.md 2): the V^T scatter cost 110 / 275 us of a 1.53 / 1.65 ms launch, the kernels are equal or faster.
        rows_path = self.attn_rows and not fp8 and (not g or (not ws and gg == 64) or win16)
        # Window blocks whose qkv weight is one plane (at most the V rows carry a second one): the GEMMs walk the REAL tokens in
        # image order and their epilogue scatters q / k rows and V^T slots into window order (LA_MAP_WINDOW_PART) - the padded
        # tokens (16 % of the rows at 64 x 64 / 14) are never multiplied.  Their q / k / v are the bias (pad-after-norm), constant
        # per block: every window block owns its buffers, filled once when they are created.
        scatter = win16 and "qkv" not in self.precise and nb * t > bn * rpg
        form = "rows" if rows_path else "fp8" if fp8 else "scatter" if scatter else "vt"
        sfx = "" if not g else ".r" if rows_path else ".w" if ws else ".g"       # (SAM: the forms and block kinds differ in buffer shapes)
        return AttnGeo(pfx=pfx, sfx=sfx, bn=bn, rpg=rpg, heads=spec.heads, hdp=hdp, scale=spec.head_dim ** -0.5, g=g, ws=ws, nb=nb, t=t,
                       gg=gg, tpad=_ceil(16 * gg, 64) if win16 else _ceil(t, 64), win16=win16, form=form,
                       arows=bn * rpg if rows_path else nb * t, o_chunks=nb // bn * (_ceil(t, 128) // 128))

    def _qkv(self, bp: str, i: int, at: AttnGeo, x: Tensor, mr: Optional[Tensor] = None):
        """The q | k | v GEMM of block i in the layout its attention reads; returns (qkv, V^T or None).  mr: the (mean, rstd) rows of a
        folded LayerNorm - the gamma-folded weight, normalised in the epilogue (rows form only)."""
        p, ea, heads, hdp = self.p, at.ea, at.heads, at.hdp
        if at.form == "rows":
            qkv = self.buf(f"{at.pfx}.qkv{at.sfx}", (at.arows, 3 * ea))
            if mr is not None:
                L.gemm(x, p[bp + ".qkv.wn"], bias=p[bp + ".qkv.bn"], out16=qkv, nstat_in=mr, ncol=p[bp + ".qkv.cn"])
            else:
                self.qkv_gemm(x, bp + ".qkv.w", qkv, None, ea)
            return qkv, None
        vtkw = dict(vt_T=at.t, vt_Tpad=at.tpad, vt_hd=hdp, vt_heads=heads, vt_ws=at.gg if at.win16 else 0)
        if at.form == "scatter":
            qb, nwy = p[bp + ".qkv.b"], at.nwy

            def fill_qk(tq):
                tq[:, : 2 * ea] = qb[: 2 * ea].to(tq.dtype)

            def fill_v(tv):
                tv.zero_()
                tv.view(at.nb, heads, hdp, at.tpad)[..., : 16 * at.gg].view(at.nb, heads, hdp, at.gg, 16)[..., :at.gg] = \
                    qb[2 * ea:].view(1, heads, hdp, 1, 1).to(tv.dtype)

            qkv = self.arena.get(f"enc.qkv.w{i}", (at.arows, 3 * ea), self.dt, False, fill_qk)
            vt = self.arena.get(f"enc.vt.w{i}", (at.nb * heads, hdp, at.tpad), self.dt, False, fill_v)
            self.qkv_gemm(x, bp + ".qkv.w", qkv, vt, ea, rowmap=(L.MAP_WINDOW_PART, (at.ws, nwy, nwy, at.g, at.g)), **vtkw)
        else:
            qkv = self.buf(f"{at.pfx}.qkv{at.sfx}", (at.arows, 3 * ea))
            vt = self.buf(f"{at.pfx}.vt{at.sfx}", (at.nb * heads, hdp, at.tpad), zero=True)
            self.qkv_gemm(x, bp + ".qkv.w", qkv, vt, ea, **vtkw)
        return qkv, vt

    def _attention(self, bp: str, at: AttnGeo, qkv: Tensor, vt: Optional[Tensor], opart: Optional[Tensor]):
        """softmax(q k^T [+ rel-pos]) v of one block in the form ``_attn_geo`` chose.  Returns (output, chunks): the output in image order
        (rows form) or in the order of qkv, and the column-sum partials per image the attention kernel left in opart (0: none)."""
        p, nb, heads, t, tpad, gg, ea, scale = self.p, at.nb, at.heads, at.t, at.tpad, at.gg, at.ea, at.scale
        tabs = dict(tabh=p[bp + ".tabh"], tabw=p[bp + ".tabw"]) if at.g else {}
        mode = L.ATTN_RELPOS_WIN16 if at.win16 else L.ATTN_RELPOS if at.g else L.ATTN_PLAIN
        ao = self.buf(f"{at.pfx}.ao{at.sfx}", (at.arows, ea))
        if at.form == "rows":
            fused_o = opart is not None and (not at.ws or self.win_fused_cs)
            wkw = dict(img_hw=(at.g, at.g), padrow=p[bp + ".qkv.pad16"]) if at.ws else {}
            L.attn_fwd_rows(qkv, ao, nb, heads, t, tpad, gg, ea, scale, mode, cspart=opart if fused_o else None, **tabs, **wkw)
        elif at.form == "fp8":
            fused_o = False
            qk8 = self.arena.get(at.pfx + ".qk8", (at.arows, 2 * ea), torch.uint8, False)
            L.qk_fp8(qkv, ea, qk8)
            L.attn_fwd_fp8(qk8, vt, ao, nb, heads, t, tpad, ea, scale)
        else:
            # column sums of the attention output from the attention kernel itself where that is cheaper than a pass over the output:
            # 260 VALU operations per wave at the end of >= 15 key tiles (global blocks: +2 %), not of a window's 4 (+30 %, measured)
            fused_o = opart is not None and (not at.g or (not at.win16 and gg > 16))
            relh = relw = None
            if not (at.win16 or gg <= 16 or gg == 64):      # (else the rel-pos terms are computed inside the attention kernel)
                relh = self.f32(f"enc.relh{at.sfx}", (nb * heads, t, gg))
                relw = self.f32(f"enc.relw{at.sfx}", (nb * heads, t, gg))
                L.relpos_terms(qkv, nb, heads, gg, ea, p[bp + ".tabh"], p[bp + ".tabw"], relh, relw)
                tabs = {}
            if fused_o:
                L.attn_fwd_cs(qkv, vt, ao, relh, relw, nb, heads, t, tpad, gg, ea, scale, mode, opart, **tabs)
            else:
                L.attn_fwd(qkv, vt, ao, relh, relw, nb, heads, t, tpad, gg, ea, scale, mode, **tabs)
        return ao, at.o_chunks if fused_o else 0

    def _block_plain(self, i: int, nm: BlockNames, at: AttnGeo, res: Tensor, x16: Tensor, rvec: Optional[Tensor], want16: bool = False):
        """Block i, a pre-LN transformer block, on the fp32 stream ``res`` with the LayerNorm kernels: norm1, q | k | v, attention, token-mean
        correction (into the pending rvec), proj, norm2, lin1 (GELU), lin2.  x16: the 16-bit operand buffer of the GEMMs.  want16: lin2 also
        writes - and the block returns - a 16-bit copy of the stream."""
        w, bp, rpg = self.w32, nm.prefix.format(i), at.rpg
        rows, e = res.shape
        xpart, opart = self.mean_parts(at, e)
        ckw = dict(colsum_part=xpart) if xpart is not None else {}
        xin, wkw = x16, {}
        if at.parted and at.form != "scatter":       # the LayerNorm partitions the rows into windows; padded tokens stay zero
            xin, wkw = self.buf("enc.xwin", (at.arows, e), zero=True), dict(window=at.ws, H=at.g, W=at.g)
        self.ln(res, f"{bp}.{nm.norm1}", nm.eps, rvec, rpg, out16=xin, **wkw, **ckw)
        qkv, vt = self._qkv(bp, i, at, xin)
        if self.kind.rope:
            self._rope(at, qkv)
        ao, o_chunks = self._attention(bp, at, qkv, vt, opart)
        if rvec is not None:
            self.mean_fix(bp, at, e, xpart, opart, o_chunks, ao, rvec)
        # (window order: window_unpartition as a row gather on the A operand - again only the real tokens are computed)
        ukw = dict(M=rows, amap=L.MAP_WINDOW_PART, p=(at.ws, at.nwy, at.nwy, at.g, at.g)) if at.parted else {}
        self.gemm_w(ao, bp + ".proj.w", bias=w[f"{bp}.{nm.proj}.bias"], res=res, out32=res, **ukw)
        self.ln(res, f"{bp}.{nm.norm2}", nm.eps, rvec, rpg, out16=x16)
        hbuf = self.buf(at.pfx + ".mlp", (rows, self.cfg.encoder_spec.mlp))
        self.gemm_w(x16, bp + ".lin1.w", bias=w[f"{bp}.{nm.lin1}.bias"], out16=hbuf, act=L.ACT_GELU)
        last16 = self.buf("enc.last16", (rows, e)) if want16 else None
        self.gemm_w(hbuf, bp + ".lin2.w", bias=w[f"{bp}.{nm.lin2}.bias"], res=res, out32=res, out16=last16)
        return last16

    # ---- LayerNorm folded into its neighbour GEMMs (norm_fold) -------------------------------------------------------------------------
    def _fold_bufs(self, tag: str, rows: int, e: int):
        """(partial row sums of the producer GEMMs, (mean, rstd) rows of the consumer GEMMs - padded to whole 256-row tiles)."""
        return self.f32(tag + ".npart", (rows, e // 64, 2)), self.f32(tag + ".nmr", (_ceil(rows, 256), 2), zero=True)

    def _planes_to_f32(self, xs: Tensor, name: str) -> Tensor:
        """hi + lo of a plane-pair stream as an fp32 matrix (the callers that leave the folded path: final LayerNorm, un-split necks)."""
        e = xs.shape[1] // 2
        out = self.f32(name, (xs.shape[0], e))
        out.copy_(xs[:, :e])
        out.add_(xs[:, e:])
        return out

    def _block_fold(self, i: int, nm: BlockNames, at: AttnGeo, xs: Tensor, part: Tensor, mr: Tensor, have_mr: bool) -> None:
        """_block_plain without LayerNorm passes (image_encoder.py:110-131,179-197; transformers ViTLayer): every residual GEMM is the
        PRODUCER of the next LayerNorm's input, q | k | v and lin1 are its CONSUMERS (gamma-folded weights, normalisation in the epilogue);
        the token-mean correction of a block joins the stream in the proj epilogue.  The residual stream itself is a pair of fp16 planes
        xs = [hi | lo] (same bytes as fp32, ~22 mantissa bits): the producers read-modify-write it in place and the hi plane IS the
        consumers' operand - no separate 16-bit copy (a producer epilogue is bound by HBM round trips: the copy's 2 E bytes per row were
        + 20 % on proj, + 8 % on lin2).  part / mr: _fold_bufs; have_mr: the stack's entry already left this block's (mean, rstd) in mr."""
        w, p, bp, rpg = self.w32, self.p, nm.prefix.format(i), at.rpg
        rows, e = xs.shape[0], xs.shape[1] // 2
        hi, lo = xs[:, :e], xs[:, e:]
        xpart, opart = self.mean_parts(at, e)
        vm = xpart is not None
        if vm or not have_mr:
            L.norm_finalize(None if have_mr else part, rows, e, nm.eps, mr, x16=hi if vm else None, rpg=rpg, cs_part=xpart)
        qkv, _ = self._qkv(bp, i, at, hi, mr)
        if self.kind.rope:
            self._rope(at, qkv)
        ao, o_chunks = self._attention(bp, at, qkv, None, opart)
        dr = self._fold_mean(bp, at, e, xpart, opart, o_chunks, ao)
        L.gemm(ao, p[bp + ".proj.w"], bias=w[f"{bp}.{nm.proj}.bias"], out16=hi, aux16=lo, nstat_out=part, rvec=dr,
               rvec_rpg=rpg if dr is not None else 0, a_kmod=self.kmod.get(bp + ".proj.w", 0))
        L.norm_finalize(part, rows, e, nm.eps, mr)
        hbuf = self.buf(at.pfx + ".mlp", (rows, self.cfg.encoder_spec.mlp))
        L.gemm(hi, p[bp + ".lin1.wn"], bias=p[bp + ".lin1.bn"], out16=hbuf, act=L.ACT_GELU, nstat_in=mr, ncol=p[bp + ".lin1.cn"])
        L.gemm(hbuf, p[bp + ".lin2.w"], bias=w[f"{bp}.{nm.lin2}.bias"], out16=hi, aux16=lo, nstat_out=part,
               a_kmod=self.kmod.get(bp + ".lin2.w", 0))

    # ---- SAM ViTDet encoder (image_encoder.py:110-131,179-197,200-255) ------------------------------------------------------------------
    def sam_encoder(self, images: Tensor, want_last_block: bool = False):
        spec: EncoderSpec = self.cfg.encoder_spec
        self._check_encoder_input(images)
        pre, nm = "image_encoder", SAM_BLOCK
        bn, _, s, _ = images.shape
        if s != spec.img_size:
            raise ValueError(f"SAM encoder expects {spec.img_size}x{spec.img_size} inputs, got {s}")
        e, g, ws = spec.dim, s // spec.patch, spec.window
        hw = g * g
        rows = bn * hw
        w, p = self.w32, self.p
        images = images.contiguous()
        geo = {True: self._attn_geo("enc", bn, hw, g), False: self._attn_geo("enc", bn, hw, g, ws)}      # by "is a global block"
        a, akw = self.patches("enc.patchA", images, rows, spec.patch)
        pkw = dict(bias=w[pre + ".patch_embed.proj.bias"], res=p[pre + ".pos"], res_mod=hw, **akw)
        # (the producer epilogue adds the per-image correction to groups of whole row tiles or of >= 128 rows: smaller grids keep the kernels)
        if self.norm_fold and self.attn_rows and ws <= 16 and (g == 64 or not spec.global_idx) and (hw % 256 == 0 or hw >= 128):
            xs = self.buf("enc.xs", (rows, 2 * e), torch.float16)          # the stream: [hi | lo]
            part, mr = self._fold_bufs("enc", rows, e)
            have_mr = hw % 256 != 0
            if not have_mr:     # (plane pairs straight from the patch embedding's epilogue: no fp32 matrix is written at all)
                L.gemm(a, p[pre + ".patch.w"], out16=xs[:, :e], aux16=xs[:, e:], nstat_out=part, **pkw)
            else:       # (a position table that is not whole row tiles: planes and statistics from a pass each, once)
                res32 = self.f32("enc.res", (rows, e))
                L.gemm(a, p[pre + ".patch.w"], out32=res32, **pkw)
                L.add_rowvec_split(res32, None, hw, xs)
                L.norm_stats(res32, nm.eps, self.buf("enc.x16", (rows, e)), mr)
            for i in range(spec.depth):
                self._block_fold(i, nm, geo[i in spec.global_idx], xs, part, mr, have_mr and i == 0)
            return self._sam_exit(bn, g, want_last_block, xs=xs)
        res = self.f32("enc.res", (rows, e))
        L.gemm(a, p[pre + ".patch.w"], out32=res, **pkw)
        x16 = self.buf("enc.x16", (rows, e))
        last16 = rvec = None
        if self.mean_planes:           # pending per-image corrections of the single-plane V / proj weights (PRECISE_WIDE)
            rvec = self.f32("enc.rvec", (bn, e), zero=True)
            rvec.zero_()
        for i in range(spec.depth):
            want16 = i == spec.depth - 1 and not (self.cfg.use_vit_sam_neck and "neck" in self.precise) and rvec is None
            last16 = self._block_plain(i, nm, geo[i in spec.global_idx], res, x16, rvec, want16)
        return self._sam_exit(bn, g, want_last_block, res=res, rvec=rvec, last16=last16)

    def _sam_exit(self, bn: int, g: int, want_last_block: bool, res: Optional[Tensor] = None, rvec: Optional[Tensor] = None,
                  last16: Optional[Tensor] = None, xs: Optional[Tensor] = None):
        """The stream leaves the SAM block stack - fp32 ``res`` with the pending ``rvec`` and, where lin2 wrote one, its 16-bit copy, or the
        folded stack's planes ``xs`` - through the neck (or as it is).  Returns (out32, out16, channels), with want_last_block also the
        last block's fp32 output."""
        spec: EncoderSpec = self.cfg.encoder_spec
        pre, e, hw = "image_encoder", spec.dim, g * g
        neck = self.cfg.use_vit_sam_neck
        split_neck = neck and (pre + ".neck.0.ws") in self.p
        if xs is not None:             # folded stack: hi is the 16-bit copy, and the neck's 1 x 1 convolution takes the pair as it stands
            last16 = xs[:, :e]
            if want_last_block or not split_neck:
                res = self._planes_to_f32(xs, "enc.res")
            if not neck:
                last16 = self.buf("enc.last16", last16.shape)
                last16.copy_(xs[:, :e])
            if not split_neck:
                xs = None
        else:
            if split_neck:             # the stream's last pass also leaves it as fp16 plane pairs: the neck's 1 x 1 conv operand
                # (range: the pair [hi | lo] holds |x| <= 131008 - la_add_rowvec_split saturates beyond, it never emits inf / NaN; SAM
                # checkpoints keep the un-normalised stream three orders of magnitude below that)
                xs = self.buf("enc.res_split", (res.shape[0], 2 * e), torch.float16)
                L.add_rowvec_split(res, rvec, hw, xs)
            elif rvec is not None:     # the stream leaves the block stack: fold the pending corrections in
                L.add_rowvec(res, rvec, hw)
            if rvec is not None and not (neck and "neck" in self.precise):
                last16 = self.buf("enc.last16", res.shape)
                L.add_cast(res, out16=last16, dt=self.dti)
        if neck:
            out = (self.conv_neck(pre + ".neck", last16, bn, g, "enc.neck", x32=res, xs=xs), None, spec.out_chans)
        else:
            out = (res, last16, e)
        return (out, res) if want_last_block else out

    # ---- plain ViT encoders: HuggingFace ViT (transformers ViTModel maths; build_encoder.py:83-100), DINOv2 (Dinov2Model) and DINOv3
    # (DINOv3ViTModel; parameters/trainval/coco/dinov3.yaml trains on its embeddings).  What differs between them is data: EncoderKind ----
    def _hf_pos(self, g: int) -> Tensor:
        """The position table at a g x g grid, [1 + g * g, E]; leaves the prefix row cls_token + pos[0], [1, E], in ``_hfpos_cache[-g]``."""
        t = self._hfpos_cache.get(g)
        if t is None:
            spec = self.cfg.encoder_spec
            pos = self.w32["image_encoder.embeddings.position_embeddings"]
            if g != spec.pos_grid:  # bicubic resample of the patch positions (constant per resolution)
                e = pos.shape[-1]
                bt = bicubic_matrix_t(spec.pos_grid, g, pos.device)                        # [gin^2, gout^2]
                grid = torch.zeros(g * g, e, device=pos.device)
                L.gemm_tn(bt, pos[0, 1:].contiguous(), grid)                               # grid = B . pos  (exact-fp32 MFMA)
                pos = torch.cat([pos[:, :1], grid.unsqueeze(0)], dim=1)
            t = pos[0].contiguous()
            self._hfpos_cache[g] = t
            self._hfpos_cache[-g] = (self.w32["image_encoder.embeddings.cls_token"][0] + t[:1]).contiguous()
        return t

    def _rope(self, at: AttnGeo, qkv: Tensor) -> None:
        """Rotate q and k of the patch rows of one block's q | k | v buffer in place (la_rope_qk), between ``_qkv`` and ``_attention``."""
        spec: EncoderSpec = self.cfg.encoder_spec
        if at.parted:
            raise NotImplementedError("la_rope_qk walks image-order rows; window-partitioned attention has no rotary form")
        hw = at.rpg - spec.prefix_tokens
        g = math.isqrt(hw)
        tab = self._rope_cache.get(g)
        if tab is None:
            tab = self._rope_cache[g] = tuple(t.to(self.dev) for t in rope_table(g, spec.head_dim, spec.rope_theta))
        L.rope_qk(qkv, at.rpg, spec.prefix_tokens, at.heads, spec.head_dim, at.hdp, tab[0], tab[1])

    def vit_encoder(self, images: Tensor):
        """``prefix_tokens`` constant rows (CLS, registers) in front of every image's patch rows, the position table where the kind has
        one, the block stack (plain or folded; la_rope_qk and the folded LayerScale are the blocks' business), the final LayerNorm; the
        prefix rows are dropped on the way out."""
        spec: EncoderSpec = self.cfg.encoder_spec
        self._check_encoder_input(images)
        pre, kind, nm, npre = "image_encoder", self.kind, self.block_names, spec.prefix_tokens
        bn, _, s, s2 = images.shape
        if kind.square and s != s2:
            raise NotImplementedError(f"the {kind.square} encoder is built for square inputs, got {s} x {s2}")
        e, g = spec.dim, s // spec.patch
        hw = g * g
        t = hw + npre
        rows = bn * t
        w, p = self.w32, self.p
        poskw = dict(res=self._hf_pos(g), res_mod=t) if kind.pos_table else {}
        prefix = self._hfpos_cache[-g] if kind.pos_table else p[pre + ".prefix"]
        images = images.contiguous()
        a, akw = self.patches("vit.patchA", images, bn * hw, spec.patch)
        res = self.f32("vit.res", (rows, e))
        res.view(bn, t, e)[:, :npre].copy_(prefix)       # CLS (+ pos[0]) and register rows (weights only; plain copy)
        L.gemm(a, p[pre + ".patch.w"], bias=w[f"{pre}.{kind.patch}.bias"], **poskw, out32=res, map=L.MAP_GROUP, p=(hw, t, npre, 0, 0), **akw)
        x16 = self.buf("vit.x16", (rows, e))
        at = self._attn_geo("vit", bn, t)
        rvec = None
        self.last_block_path = "fold" if self.norm_fold and at.form == "rows" and t >= 128 else "plain"
        if self.last_block_path == "fold":                          # (per-image groups of the producer epilogue: >= 128 rows)
            # The stream enters through a row map (prefix gap), so its planes and first statistics come from one pass each; the final
            # LayerNorm is the LayerNorm kernel on hi + lo.
            xs = self.buf("vit.xs", (rows, 2 * e), torch.float16)
            part, mr = self._fold_bufs("vit", rows, e)
            L.add_rowvec_split(res, None, t, xs)
            L.norm_stats(res, nm.eps, x16, mr)
            for i in range(spec.depth):
                self._block_fold(i, nm, at, xs, part, mr, i == 0)
            res = self._planes_to_f32(xs, "vit.res")
        else:
            if self.mean_planes:
                rvec = self.f32("vit.rvec", (bn, e), zero=True)
                rvec.zero_()
            for i in range(spec.depth):
                self._block_plain(i, nm, at, res, x16, rvec)
        fin = self.f32("vit.final", (rows, e))
        fin16 = self.buf("vit.final16", (rows, e))
        self.ln(res, f"{pre}.{kind.final_norm}", nm.eps, rvec, t, out32=fin, out16=fin16)
        out32 = self.f32("vit.out32", (bn * hw, e))
        out16 = self.buf("vit.out16", (bn * hw, e))
        out32.view(bn, hw, e).copy_(fin.view(bn, t, e)[:, npre:])      # drop the prefix rows (plain strided copy)
        out16.view(bn, hw, e).copy_(fin16.view(bn, t, e)[:, npre:])
        return out32, out16, e

    def encode_images(self, images: Tensor):
        """(Bn,3,S,S) fp32 -> (emb32 [Bn*hw, C] NHWC fp32, emb16 or None, C, g)."""
        spec = self.cfg.encoder_spec
        if spec is None:
            raise ValueError("this model was built without an image encoder (use_vit=False)")

        _ = self.kind          # raises for an unknown kind
        out32, out16, c = self.sam_encoder(images) if spec.kind == "sam" else self.vit_encoder(images)
        return out32, out16, c, images.shape[-1] // spec.patch

    def lam_neck(self, emb32: Tensor, emb16: Optional[Tensor], bn: int, g: int) -> Tensor:
        if "neck" in self.precise:
            return self.conv_neck("neck", None, bn, g, "lamneck", x32=emb32)
        if emb16 is None:
            emb16 = self.buf("neck.in16", tuple(emb32.shape))
            L.add_cast(emb32, out16=emb16, dt=self.dti)
        return self.conv_neck("neck", emb16, bn, g, "lamneck")

    # ------------------------------------------------------------------------------------------------
    # decoder attention building blocks
    # ------------------------------------------------------------------------------------------------
    def _attn_core(self, q32, k32, v32, groups, nq, nk, internal, tag, image_side: bool = False) -> Tensor:
        """image_side: the output feeds an image-side GEMM (rows = groups * hw): plane-pair operand in split mode."""
        heads = self.cfg.dec_heads
        o16 = self.ibuf(tag + ".o16", groups * nq, internal) if image_side else self.dbuf(tag + ".o16", (groups * nq, internal))
        L.attn_small(q32, k32, v32, groups, nq, nk, heads, internal // heads, out16=o16, dt=self.idti if image_side else self.ddti)
        return o16

    def attention_mlp_block(self, pre: str, x32: Tensor, groups: int, n: int, tag: str) -> Tensor:
        """AttentionMLPBlock (common.py:151-184): y = LN(attn(x)+x); out = LN(mlp(y)+y), one shared LayerNorm, GELU."""
        p = self.p
        rows, d = x32.shape
        internal = p[pre + ".attn.q_proj.w"].shape[0]
        x16 = self.dbuf(tag + ".x16", (rows, d))
        L.add_cast(x32, out16=x16, dt=self.ddti)
        qkv = self.f32(tag + ".qkv", (rows, 3 * internal))
        L.gemm(x16, p[pre + ".attn.qkv.w"], bias=p[pre + ".attn.qkv.b"], out32=qkv)
        o16 = self._attn_core(qkv[:, :internal], qkv[:, internal:2 * internal], qkv[:, 2 * internal:], groups, n, n, internal, tag)
        y = self.f32(tag + ".y", (rows, d))
        y16 = self.dbuf(tag + ".y16", (rows, d))
        self._token_sublayer(o16, pre + ".attn.out_proj", pre + ".norm", x32, y, y, y16)
        z = self.f32(tag + ".z", (rows, d))
        self._token_mlp(y16, pre + ".mlp", L.ACT_GELU, tag + ".h", pre + ".norm", y, z, z, None)
        return z

    def _token_sublayer(self, a: Tensor, mod: str, norm: str, res, tnew: Tensor, t32: Tensor, t16, tq16=None, tpe=None) -> None:
        """End of a token-side sub-layer (transformer.py:303-320, 248-250, 146-152; common.py:176-183): tnew = a W^T + b of ``mod`` (+ res),
        (t32, t16) = LayerNorm ``norm`` of it as fp32 / GEMM operand; tq16: the operand copy of t32 + tpe (tokens + their PE) as well."""
        w = self.w32
        L.gemm(a, self.p[mod + ".w"], bias=w[mod + ".bias"], res=res, out32=tnew)
        L.layernorm(tnew, w[norm + ".weight"], w[norm + ".bias"], 1e-5, out32=t32, out16=t16, out16_pe=tq16, pe=tpe, dt=self.ddti)

    def _token_mlp(self, x16: Tensor, mlp: str, act: int, hname: str, norm: str, res, tnew: Tensor, t32: Tensor, t16, tq16=None, tpe=None):
        """Token-side MLP sub-layer (transformer.py:317-320, 149-152; common.py:181-183): lin1 + ``act`` into the 16-bit hidden buffer
        ``hname``, then lin2 + res and the norm as in ``_token_sublayer``."""
        hbuf = self.dbuf(hname, (x16.shape[0], self.cfg.dec_mlp))
        L.gemm(x16, self.p[mlp + ".lin1.w"], bias=self.w32[mlp + ".lin1.bias"], out16=hbuf, act=act)
        self._token_sublayer(hbuf, mlp + ".lin2", norm, res, tnew, t32, t16, tq16, tpe)

    def fused_ok(self, nt: int) -> bool:
        return self.fuse_twoway and nt <= 32

    def pe_table(self, proj: str, pe32: Tensor) -> Tensor:
        """pe W^T + b of one image-side projection, [hw, internal] fp32: the positional encoding's share of (x + pe) W^T + b is a constant
        of (weights, grid), computed once per engine and grid (exact-fp32 MFMA) and added inside the fused two-way kernels."""
        key = (proj, pe32.shape[0])
        t = self._pe_tables.get(key)
        if t is None:
            t = torch.empty(pe32.shape[0], self.w32[proj + ".weight"].shape[0], device=self.dev)
            L.gemm(pe32, self.w32[proj + ".weight"], bias=self.w32[proj + ".bias"], out32=t)
            t = L.twoway_pe_layout(t)            # in the order the tile kernels read it (la_twoway_pe_layout)
            self._pe_tables[key] = t
        return t

    def _t2i(self, ca: str, tq16: Tensor, img32: Tensor, pe32: Tensor, img16, imgpe16, groups: int, nt: int, hw: int, tag: str) -> Tensor:
        """Attention output (before out_proj) of the tokens, queries from tq16 = tokens + PE, over the image side (transformer.py:310-313,
        245-248); fused: K / V are never materialised."""
        w, p, di, ri = self.w32, self.p, self.cfg.embed_dim // 2, groups * hw
        q = self.f32(tag + ".tq", (groups * nt, di))
        L.gemm(tq16, p[ca + ".q_proj.w"], bias=w[ca + ".q_proj.bias"], out32=q)
        if self.fused_ok(nt):
            o = self.f32(tag + ".t2i.o", (groups * nt, di))
            part = self.f32(tag + ".t2i.part", (L.twoway_part_size(groups, hw, nt, self.cfg.embed_dim),))
            L.twoway_t2i(img32, p[ca + ".k_proj.planes"], p[ca + ".v_proj.planes"], self.pe_table(ca + ".k_proj", pe32), w[ca + ".v_proj.bias"], q,
                         groups, hw, nt, self.cfg.dec_heads, part, o)
            return o
        k, v = self.f32(tag + ".ik", (ri, di)), self.f32(tag + ".iv", (ri, di))
        self.igemm(imgpe16, ca + ".k_proj.w", bias=w[ca + ".k_proj.bias"], out32=k)
        self.igemm(img16, ca + ".v_proj.w", bias=w[ca + ".v_proj.bias"], out32=v)
        return self._attn_core(q, k, v, groups, nt, hw, di, tag + ".t2i")

    def two_way(self, pre: str, tok32: Tensor, groups: int, nt: int, img32: Tensor, img16, imgpe16, hw: int,
                pe32: Tensor, tag: str, want_tokens: bool):
        """TwoWayTransformer (transformer.py:206-329).  tok32 [groups*nt, D] fp32 (also the token PE); image side
        [groups*hw, D] as fp32 stream, updated in place (+ its GEMM-operand copies x and x+pe when the unfused chain runs:
        ``fused_ok(nt)`` false).  Returns (tokens32, tokens16)."""
        w, p = self.w32, self.p
        d = self.cfg.embed_dim
        r = groups * nt
        fused = self.fused_ok(nt)
        tpe = tok32
        t32 = self.f32(tag + ".t32", (r, d))
        t16 = self.dbuf(tag + ".t16", (r, d))
        tq16 = self.dbuf(tag + ".tq16", (r, d))
        tnew = self.f32(tag + ".tnew", (r, d))
        for l in range(2):
            lp = f"{pre}.layers.{l}"
            sa = lp + ".self_attn"
            if l == 0:
                L.add_cast(tok32, out16=t16, dt=self.ddti)
                qkv = self.f32(tag + ".sa_qkv", (r, 3 * d))
                L.gemm(t16, p[sa + ".qkv.w"], bias=p[sa + ".qkv.b"], out32=qkv)
                o16 = self._attn_core(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], groups, nt, nt, d, tag + ".sa")
            else:
                qk = self.f32(tag + ".sa_qk", (r, 2 * d))
                L.gemm(tq16, p[sa + ".qk.w"], bias=p[sa + ".qk.b"], out32=qk)
                v = self.f32(tag + ".sa_v", (r, d))
                L.gemm(t16, p[sa + ".v_proj.w"], bias=w[sa + ".v_proj.bias"], out32=v)
                o16 = self._attn_core(qk[:, :d], qk[:, d:], v, groups, nt, nt, d, tag + ".sa")
            # (layer 0's self-attention has no residual: its output replaces the tokens)
            self._token_sublayer(o16, sa + ".out_proj", lp + ".norm1", t32 if l else None, tnew, t32, t16, tq16, tpe)
            # tokens -> image
            ca = lp + ".cross_attn_token_to_image"
            o16 = self._t2i(ca, tq16, img32, pe32, img16, imgpe16, groups, nt, hw, tag)
            self._token_sublayer(o16, ca + ".out_proj", lp + ".norm2", t32, tnew, t32, t16)
            # MLP (ReLU)
            self._token_mlp(t16, lp + ".mlp", L.ACT_RELU, tag + ".mlp", lp + ".norm3", t32, tnew, t32, t16, tq16, tpe)
            # image -> tokens; the norm leaves x and x + pe up to date for the next layer
            self._image_from_tokens(lp + ".cross_attn_image_to_token", lp + ".norm4", True, fused, tq16, t16, "", img32, img16, imgpe16, pe32,
                                    groups, nt, hw, tag)
        if not want_tokens:
            return None, None
        ca = pre + ".final_attn_token_to_image"
        o16 = self._t2i(ca, tq16, img32, pe32, img16, imgpe16, groups, nt, hw, tag)
        self._token_sublayer(o16, ca + ".out_proj", pre + ".norm_final_attn", t32, tnew, t32, t16)
        return t32, t16

    def _image_from_tokens(self, ca: str, norm: str, refresh_pe: bool, fused: bool, tk16: Tensor, tv16: Tensor, kv: str, img32: Tensor,
                           img16, imgpe16, pe32: Tensor, groups: int, nt: int, hw: int, tag: str) -> None:
        """Image <- tokens attention of a TwoWayAttentionBlock (transformer.py:322-327) / OneWayAttentionBlock (transformer.py:143-147):
        k / v from the token operands tk16 / tv16 into the buffers tag.tk<kv> / tag.tv<kv>, then in place on the fp32 stream
        img = LayerNorm ``norm`` (img + out_proj(attn(q = img + pe, k, v))).  fused: one la_twoway_i2t.  Otherwise the chain on the operand
        copies: q from imgpe16 (x + pe); the norm writes img16 (x) and, with refresh_pe, imgpe16 for the next attention that reads it."""
        w, p = self.w32, self.p
        di = self.cfg.embed_dim // 2
        kt, vtok = self.f32(f"{tag}.tk{kv}", (groups * nt, di)), self.f32(f"{tag}.tv{kv}", (groups * nt, di))
        L.gemm(tk16, p[ca + ".k_proj.w"], bias=w[ca + ".k_proj.bias"], out32=kt)
        L.gemm(tv16, p[ca + ".v_proj.w"], bias=w[ca + ".v_proj.bias"], out32=vtok)
        if fused:       # q_proj + attention + out_proj + residual + norm
            L.twoway_i2t(img32, p[ca + ".q_proj.planes"], self.pe_table(ca + ".q_proj", pe32), kt, vtok, p[ca + ".out_proj.planes"],
                         w[ca + ".out_proj.bias"], w[norm + ".weight"], w[norm + ".bias"], 1e-5, groups, hw, nt, self.cfg.dec_heads)
            return
        qi = self.f32(tag + ".iq", (groups * hw, di))
        self.igemm(imgpe16, ca + ".q_proj.w", bias=w[ca + ".q_proj.bias"], out32=qi)
        oi16 = self._attn_core(qi, kt, vtok, groups, hw, nt, di, tag + ".i2t", image_side=True)
        self.igemm(oi16, ca + ".out_proj.w", bias=w[ca + ".out_proj.bias"], res=img32, out32=img32)
        pe = dict(out16_pe=imgpe16, pe=pe32, pe_mod=hw) if refresh_pe else {}
        L.layernorm(img32, w[norm + ".weight"], w[norm + ".bias"], 1e-5, out32=img32, out16=img16, dt=self.idti, **pe)

    # la_stream_mlp against the lin1 -> lin2 (+ residual) -> LayerNorm chain on the same buffers (tools/bench_oneway.py, part (a);
    # profiles/r12_oneway.md has the table).  A 128-row tile takes 223 us whatever the row count up to 32 768 rows (one workgroup per CU);
    # the chain takes 186 us at 900 rows, 212 us at 4 096, 253 us at 7 200 (kernel 1.14x faster, spreads apart), 610 us at 32 768 (2.5x).
    # The fused kernel is used from the smallest measured row count at which it wins, the chain below.
    ONEWAY_MLP_MIN_ROWS = 7200

    def oneway_fused(self, nt: int) -> bool:
        return self.fuse_oneway and self.fused_ok(nt)

    def oneway_mlp_fused(self, nt: int, rows: int) -> bool:
        return self.oneway_fused(nt) and rows >= self.ONEWAY_MLP_MIN_ROWS

    def one_way(self, pre: str, tok32: Tensor, groups: int, nt: int, img32: Tensor, img16, imgpe16, hw: int, pe32: Tensor, tag: str):
        """OneWayTransformer (transformer.py:26-154).  tok32 [groups*nt, D] fp32: the tokens pass through untouched and are keys and values
        of both layers WITHOUT a positional encoding and without a key mask (OneWayTransformer.forward never passes one on).  The image
        side [groups*hw, D] is the fp32 stream, updated in place; per layer
            img = norm1(img + attn(q = img + pe, k = v = tokens));    img = norm2(img + lin2(relu(lin1(img))))
        Fused (``oneway_fused(nt)``): la_twoway_i2t + la_stream_mlp, two launches a layer - the MLP half on the chain below
        ONEWAY_MLP_MIN_ROWS rows.  Otherwise the chain on the GEMM-operand copies img16 (x) and imgpe16 (x + pe), which the last norm
        leaves up to date.  norm3 is never applied.  Returns (tokens32, tokens16) for class_mlp: the class embeddings themselves."""
        w, p, cfg = self.w32, self.p, self.cfg
        d = cfg.embed_dim
        r, ri = groups * nt, groups * hw
        fused = self.oneway_fused(nt)
        mlp_fused = self.oneway_mlp_fused(nt, ri)
        t16 = self.dbuf(tag + ".t16", (r, d))
        L.add_cast(tok32, out16=t16, dt=self.ddti)
        if fused and not mlp_fused:
            img16 = self.ibuf(tag + ".x16", ri, d)
        for l in range(2):
            lp = f"{pre}.layers.{l}"
            # the tokens never change: k / v of both layers, in buffers of their own, depend on the class embeddings alone.  norm1 leaves only
            # x up to date: the MLP reads it, and norm2 below refreshes x + pe
            self._image_from_tokens(lp + ".cross_attn_image_to_token", lp + ".norm1", False, fused, t16, t16, str(l), img32, img16, imgpe16,
                                    pe32, groups, nt, hw, tag)
            if mlp_fused:   # lin1 + ReLU + lin2 + residual + norm2: the 2048-wide hidden layer never leaves the chip
                L.stream_mlp(img32, p[lp + ".mlp.lin1.planes"], w[lp + ".mlp.lin1.bias"], p[lp + ".mlp.lin2.planes"], w[lp + ".mlp.lin2.bias"],
                             w[lp + ".norm2.weight"], w[lp + ".norm2.bias"], 1e-5)
                continue
            if fused:
                L.add_cast(img32, out16=img16, dt=self.idti)
            if self.isplit:     # (a GEMM writes no plane pairs: the hidden layer goes through fp32)
                h32 = self.f32(tag + ".mlp32", (ri, cfg.dec_mlp))
                self.igemm(img16, lp + ".mlp.lin1.w", bias=w[lp + ".mlp.lin1.bias"], out32=h32, act=L.ACT_RELU)
                hbuf = self.ibuf(tag + ".mlp", ri, cfg.dec_mlp)
                L.add_cast(h32, out16=hbuf, dt=self.idti)
            else:
                hbuf = self.dbuf(tag + ".mlp", (ri, cfg.dec_mlp))
                self.igemm(img16, lp + ".mlp.lin1.w", bias=w[lp + ".mlp.lin1.bias"], out16=hbuf, act=L.ACT_RELU)
            self.igemm(hbuf, lp + ".mlp.lin2.w", bias=w[lp + ".mlp.lin2.bias"], res=img32, out32=img32)
            chain = {} if fused else dict(out16=img16, out16_pe=imgpe16, pe=pe32, pe_mod=hw)      # x and x + pe for the next layer's chain
            L.layernorm(img32, w[lp + ".norm2.weight"], w[lp + ".norm2.bias"], 1e-5, out32=img32, dt=self.idti, **chain)
        return tok32, t16

    # ------------------------------------------------------------------------------------------------
    # prompt encoder (prompt_encoder.py:564-827)
    # ------------------------------------------------------------------------------------------------
    def _sparse_tokens(self, b, m, c, points, boxes) -> Tuple[Tensor, int]:
        """Bookkeeping of the sparse prompt tokens -> (xy, kind, shift) device arrays.  Index work only, all on device
        (inputs are device tensors) so that the whole forward can be captured in a HIP graph."""
        dev = self.dev
        pcount = b * m * c
        parts_xy, parts_kind, parts_shift = [], [], []
        if points is not None:
            xy, lab = points
            xy = xy.reshape(pcount, -1, 2).to(dev, torch.float32)
            lab = lab.reshape(pcount, -1).to(dev)
            kind = ((lab != 0).to(torch.int32) + (lab > 0).to(torch.int32))      # 0 NULL, 1 negative, 2 positive
            shift = torch.ones_like(kind)
            if boxes is None:   # extra token at (0,0), label -1 == NEGATIVE in this code base, not shifted (prompt_encoder.py:91-95)
                xy = torch.cat([xy, torch.zeros(pcount, 1, 2, device=dev)], dim=1)
                kind = torch.cat([kind, torch.ones(pcount, 1, dtype=torch.int32, device=dev)], dim=1)
                shift = torch.cat([shift, torch.zeros(pcount, 1, dtype=torch.int32, device=dev)], dim=1)
            parts_xy.append(xy); parts_kind.append(kind); parts_shift.append(shift)
        if boxes is not None:
            bx, bf = boxes
            nb = bx.shape[3]
            corners = bx.reshape(pcount, nb * 2, 2).to(dev, torch.float32)
            kind = (torch.arange(2 * nb, device=dev, dtype=torch.int32) % 2 + 3).expand(pcount, -1)
            flags2 = bf.reshape(pcount, nb).to(dev).repeat(1, 2)            # tiled flags vs interleaved corners (:661-667)
            kind = (kind * (flags2 != 0).to(torch.int32)).contiguous()
            parts_xy.append(corners); parts_kind.append(kind); parts_shift.append(torch.ones_like(kind))
        if not parts_xy:
            xy = torch.zeros(pcount, 1, 2, device=dev)
            kind = torch.full((pcount, 1), 5, dtype=torch.int32, device=dev)
            shift = torch.zeros_like(kind)
        else:
            xy, kind, shift = torch.cat(parts_xy, 1), torch.cat(parts_kind, 1), torch.cat(parts_shift, 1)
        ns = kind.shape[1]
        return (xy.contiguous(), kind.contiguous(), shift.contiguous()), ns

    def sample_rows(self, c: int) -> Tensor:
        """RandomMatrixEncoder.sample_rows: a fresh permutation every forward, also in eval (prompt_encoder.py:245-248)."""
        return torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(self.cfg.bank_size - 1)[: c - 1] + 1])

    def prompt_encoder(self, support32: Tensor, b: int, m: int, g: int, points, boxes, masks, flag_examples: Tensor,
                       selected_rows: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """support32: [B*M*hw, D] NHWC fp32.  Returns class_embeddings (B,C,D), class_examples_embeddings (B,M,C,D),
        class_examples_src (P, hw, D) NHWC.  With cfg.pool_side = k > 1 the examples are the M k k region means and ``flag_examples``
        comes back repeated to (B, M k k, C), as the reference's result dictionary carries it.  With cfg.prompt_encoder = "TokenPool" the
        stream has one slab per support image and class_examples_src is (B*M, hw, D) (``_token_pool``)."""
        cfg, w, p = self.cfg, self.w32, self.p
        pe_ = "prompt_encoder"
        d = cfg.embed_dim
        first = points[0] if points is not None else boxes[0] if boxes is not None else masks[0] if masks is not None else None
        if first is None:
            raise ValueError("No prompts provided")
        c = first.shape[2]
        pcount = b * m * c
        hw = g * g
        # sparse tokens
        (xy, kind, shift), ns = self._sparse_tokens(b, m, c, points, boxes)
        sp = self.f32("pe.sparse0", (pcount * ns, d))
        L.point_embed(xy, kind, shift, d, cfg.image_size, w[pe_ + ".pe_layer.positional_encoding_gaussian_matrix"],
                      p[pe_ + ".type_emb"], w[pe_ + ".not_a_point_embed.weight"], w[pe_ + ".no_sparse_embedding.weight"], sp)
        sp = self.attention_mlp_block(pe_ + ".sparse_embedding_attention", sp, b * m, c * ns, "pe.sea")
        class_enc = None
        if cfg.bank_size:
            if selected_rows is None:
                selected_rows = self.sample_rows(c)
            class_enc = w[pe_ + ".class_encoder.pos_embedding"][0, 0].index_select(0, self.h2d(selected_rows)).contiguous()
            ce_rows = class_enc.repeat_interleave(ns, dim=0).contiguous()       # rows ordered (c, n)
            sp2 = self.f32("pe.sparse_ce", (pcount * ns, d))
            L.add_cast(sp, ce_rows, c * ns, out32=sp2, dt=self.ddti)
            sp = sp2
        if cfg.prompt_encoder == "TokenPool":
            return self._token_pool(support32, sp, class_enc, b, m, c, ns, g, masks, flag_examples)
        # dense stream: one slab per (support, class) pair, ns tokens each
        pe32, src32, src16, srcpe16, mk, mf, hm = self._prompt_stream(pcount, ns, pcount, g, masks)
        L.mask_embed(mk, mf, pcount, c, hm, g, d, p[pe_ + ".mask_w"], support32, class_enc, pe32, src32, src16, srcpe16, self.idti)
        self.two_way(pe_ + ".transformer", sp, pcount, ns, src32, src16, srcpe16, hw, pe32, "pe.tw", want_tokens=False)
        k = cfg.pool_side
        fe = self.h2d(flag_examples.reshape(b, m, c), torch.uint8).contiguous()
        if cfg.embedding_extraction == "cross_attention":
            emb = self.extract_embeddings(src32, b, m, c, hw)
            n = emb.shape[1]
            # prompt_encoder.py:299-300: a query of class c is valid when any support of the episode shows the class
            flags = (fe != 0).any(dim=1, keepdim=True).to(torch.uint8).expand(b, n, c).contiguous()
            return self._prompt_result(flags, None, emb, src32.view(pcount, hw, d))
        if k > 1:
            # embeddings_per_example > 1 (prompt_encoder.py:726-731): k x k region means per (support, class) instead of the slab mean; every
            # bin is an example of its own from here on - M k k of them, flagged like the support they come from
            m = m * k * k
            emb = self.f32("pe.emb", (b * m * c, d))
            L.region_mean(src32, b, m // (k * k), c, g, k, d, emb)
            fe = fe.repeat_interleave(k * k, dim=1).contiguous()
            flag_examples = fe
        else:
            emb = self.f32("pe.emb", (pcount, d))
            L.colmean(src32, pcount, hw, d, emb, self.f32("pe.colmean.part", (pcount, L.COLMEAN_SPLIT, d)))
        emb, cls = self._merge_and_class_mean(emb, fe, b, m, c)
        return self._prompt_result(flag_examples, cls, emb.view(b, m, c, d).clone(), src32.view(pcount, hw, d))

    def _prompt_stream(self, slabs: int, nt: int, pcount: int, g: int, masks):
        """The prompt encoder's dense stream, ``slabs`` slabs of g g rows that meet ``nt`` tokens each, and what la_mask_embed[_pooled]
        fills it from (prompt_encoder.py:631-644, 880-896) -> (pe32, src32, src16, srcpe16, masks (pcount, side, side) fp32, flags int32,
        side).  Without mask prompts: None, None, 0."""
        mk, mf, hm = None, None, 0
        if masks is not None:
            mk, mf = masks
            if mk.shape[-1] != mk.shape[-2]:
                raise ValueError("prompt masks must be square")
            hm = mk.shape[-1]
            mk = self.h2d(mk, torch.float32).reshape(pcount, hm, hm).contiguous()
            mf = self.h2d(mf.reshape(pcount), torch.int32).contiguous()
        return self.dense_pe(g), *self._stream_bufs("pe.src", slabs * g * g, self.fused_ok(nt)), mk, mf, hm

    def _stream_bufs(self, name: str, rows: int, fused: bool):
        """The image-side stream [rows, D] of a transformer call -> (fp32 stream, x, x + pe): the two GEMM-operand copies exist only for
        the unfused chain, the fused kernels read the fp32 stream itself."""
        d = self.cfg.embed_dim
        return (self.f32(name + "32", (rows, d)), None if fused else self.ibuf(name + "16", rows, d),
                None if fused else self.ibuf(name + "pe16", rows, d))

    @staticmethod
    def _prompt_result(flag_examples: Tensor, cls: Optional[Tensor], emb: Tensor, src: Tensor) -> Dict[str, Tensor]:
        """The prompt encoder's result dictionary (prompt_encoder.py:310-313, 746-751); embedding_extraction has no class mean: cls None."""
        res = {"flag_examples": flag_examples, "class_embeddings": cls, "class_examples_embeddings": emb, "class_examples_src": src}
        return {k: v for k, v in res.items() if v is not None}

    def _merge_and_class_mean(self, emb: Tensor, fe: Tensor, b: int, m: int, c: int):
        """prompt_class_information_merge (the three optional merge attentions) and the flag-masked mean over the M examples
        (prompt_encoder.py:693-745) -> (emb [B*M*C, D], class_embeddings (B, C, D))."""
        cfg, d, pe_ = self.cfg, self.cfg.embed_dim, "prompt_encoder"
        if cfg.class_attention:
            emb = self.attention_mlp_block(pe_ + ".class_attention", emb, b * m, c, "pe.ca")
        if cfg.example_attention:
            e2 = emb.view(b, m, c, d).permute(0, 2, 1, 3).contiguous().view(b * c * m, d)
            e2 = self.attention_mlp_block(pe_ + ".example_attention", e2, b * c, m, "pe.ea")
            emb = e2.view(b, c, m, d).permute(0, 2, 1, 3).contiguous().view(b * m * c, d)
        if cfg.example_class_attention:
            emb = self.attention_mlp_block(pe_ + ".class_example_attention", emb, b, m * c, "pe.cea")
        cls = torch.empty(b, c, d, device=self.dev, dtype=torch.float32)
        L.class_mean(emb, fe, b, m, c, d, cls)
        return emb, cls

    def _token_pool(self, support32: Tensor, sp: Tensor, class_enc: Optional[Tensor], b: int, m: int, c: int, ns: int, g: int, masks,
                    flag_examples: Tensor) -> Dict[str, Tensor]:
        """prompt_encoder = "TokenPool" (PromptImagePoolEncoder.forward, prompt_encoder.py:880-915).  sp: the sparse tokens [B*M*C*Ns, D]
        in (c, n) order per support, class rows added.  ONE stream slab per support image - support + the class sum of the dense prompts
        (la_mask_embed_pooled) - goes through the two-way transformer with the C Ns tokens of the support; BOTH outputs are used: an
        example's embedding is the mean of its class's Ns output tokens, and class_examples_src is the image side, (B*M, hw, D)."""
        cfg, p, pe_ = self.cfg, self.p, "prompt_encoder"
        d, hw, s, nt, pcount = cfg.embed_dim, g * g, b * m, c * ns, b * m * c
        # one slab per support, c ns tokens each: above 32 tokens a support the unfused chain runs, on the GEMM-operand copies
        pe32, src32, src16, srcpe16, mk, mf, hm = self._prompt_stream(s, nt, pcount, g, masks)
        L.mask_embed_pooled(mk, mf, s, c, hm, g, d, p[pe_ + ".mask_w"], support32, class_enc, pe32, src32, src16, srcpe16, self.idti)
        t32, _ = self.two_way(pe_ + ".transformer", sp, s, nt, src32, src16, srcpe16, hw, pe32, "pe.tw", want_tokens=True)
        if ns == 1:
            emb = t32
        else:                               # "(b m) (c n) d -> b m c d", mean over n
            emb = self.f32("pe.emb", (pcount, d))
            L.colmean(t32, pcount, ns, d, emb, self.f32("pe.colmean.part", (pcount, L.COLMEAN_SPLIT, d)))
        fe = self.h2d(flag_examples.reshape(b, m, c), torch.uint8).contiguous()
        emb, cls = self._merge_and_class_mean(emb, fe, b, m, c)
        return self._prompt_result(flag_examples, cls, emb.view(b, m, c, d).clone(), src32.view(s, hw, d))

    def extract_embeddings(self, src32: Tensor, b: int, m: int, c: int, hw: int) -> Tensor:
        """embedding_extraction = "cross_attention" (EmbeddingTransformer.forward, prompt_encoder.py:289-313): n learned queries per (b, c)
        pair through two OneWayAttentionBlocks (transformer.py:140-154) over the M hw stream rows of the pair -> (B, n, C, D).  query_pe is
        zero, the activation is ReLU, norm3 is never applied, and NO key is masked: the key mask the reference builds from flag_examples
        leaves the scores untouched (common.py:120-124), so padded supports take part in the softmax exactly as there."""
        cfg, w, p = self.cfg, self.w32, self.p
        ex = "prompt_encoder.embedding_extraction"
        d, n = cfg.embed_dim, int(cfg.embeddings_per_example)
        di, bc, r = d // 2, b * c, L.EXTRACT_HEADS * n
        rows = bc * n
        t32 = self.f32("pe.xa.t32", (rows, d))
        t16 = self.dbuf("pe.xa.t16", (rows, d))
        tnew = self.f32("pe.xa.tnew", (rows, d))
        t32.view(bc, n, d).copy_(w[ex + ".embeddings.weight"])             # "n d -> (b c) n d"
        scratch = self.f32("pe.xa.part", (bc * L.extract_pool_plan(m, hw, d, r)[2],))
        pooled = self.f32("pe.xa.pooled", (bc, r, d))
        o = self.f32("pe.xa.o", (rows, di))
        for l in range(2):
            lp = f"{ex}.layers.{l}"
            ca = lp + ".cross_attn_image_to_token"
            if l == 0:
                qt = p[ex + ".qt0"]
            else:
                q = self.f32("pe.xa.q", (rows, di))
                L.gemm(t16, p[ca + ".q_proj.w"], bias=w[ca + ".q_proj.bias"], out32=q)
                qt = self.f32("pe.xa.qt", (bc, r, d))
                L.extract_fold(q, w[ca + ".k_proj.weight"], bc, n, d, qt)
            L.extract_pool(src32, qt, b, m, c, hw, d, n, scratch, pooled)
            L.extract_unfold(pooled, w[ca + ".v_proj.weight"], w[ca + ".v_proj.bias"], bc, n, d, o)
            o16 = o
            if self.ddt != torch.float32:
                o16 = self.dbuf("pe.xa.o16", (rows, di))
                L.add_cast(o, out16=o16, dt=self.ddti)
            self._token_sublayer(o16, ca + ".out_proj", lp + ".norm1", t32, tnew, t32, t16)
            self._token_mlp(t16, lp + ".mlp", L.ACT_RELU, "pe.xa.mlp", lp + ".norm2", t32, tnew, t32, t16)
        # "(b c) n d -> b n c d"; always a copy: the arena buffer is overwritten by the next forward (with n = 1 the permutation is a view)
        return t32.view(b, c, n, d).permute(0, 2, 1, 3).clone(memory_format=torch.contiguous_format)

    # ------------------------------------------------------------------------------------------------
    # mask decoder (mask_decoder.py:316-363)
    # ------------------------------------------------------------------------------------------------
    def example_valid(self, flag_examples: Tensor) -> Tensor:
        """(B, N, C) example flags -> u8 (B, C): classes with at least one valid example.  The others' low-res planes are -inf (a maximum
        over nothing); their full-resolution planes are forced to -inf as well (la_post_final's class mask) where resampling -inf
        planes would give the reference's NaN."""
        return (self.h2d(flag_examples) != 0).any(dim=1).to(torch.uint8).contiguous()

    def mask_decoder(self, query32: Tensor, b: int, g: int, class_emb: Tensor, examples: Optional[Tensor] = None,
                     flag_examples: Optional[Tensor] = None) -> Tensor:
        """query32 [B*hw, D] NHWC fp32, class_emb (B,C,D) fp32 -> low-res logits (B, C, 4g, 4g) fp32.  segment_example_logits
        (mask_decoder.py:279-287,309-313): the tokens are the N C per-example embeddings ``examples`` (B,N,C,D) in (n, c) order and every
        pixel keeps the maximum over the examples that ``flag_examples`` (B,N,C) marks valid."""
        cfg, d, hw = self.cfg, self.cfg.embed_dim, g * g
        ex = None
        if cfg.segment_example_logits:
            if examples is None or flag_examples is None:
                raise ValueError("segment_example_logits needs the per-example embeddings and their flags (class_examples_embeddings, "
                                 "flag_examples of the prompt encoder's result)")
            nex, ncls = examples.shape[1], examples.shape[2]
            ex = (nex, ncls, self.h2d(flag_examples, torch.uint8).reshape(b, nex, ncls).contiguous())
            class_emb = examples.reshape(b, nex * ncls, d)
        c = class_emb.shape[1]
        pe32 = self.dense_pe(g)
        fused = self.oneway_fused(c) if cfg.one_way else self.fused_ok(c)
        img32, img16, imgpe16 = self._decoder_stream(query32, pe32, b * hw, hw, fused)
        tok = self.h2d(class_emb, torch.float32).reshape(b * c, d).contiguous()
        if cfg.one_way:
            t32, t16 = self.one_way("mask_decoder.transformer", tok, b, c, img32, img16, imgpe16, hw, pe32, "md.ow")
        else:
            t32, t16 = self.two_way("mask_decoder.transformer", tok, b, c, img32, img16, imgpe16, hw, pe32, "md.tw", want_tokens=True)
        cls1 = None
        if cfg.classification_levels == 2:
            # coarse level (mask_decoder.py:345-346): the transformer's fp32 tokens before class_mlp against the fp32 D-channel stream
            # before the upscaler, at the grid resolution
            cls1 = self.f32("md.cls1", (b, c, g, g))
            L.classify_wide(t32, img32, b, hw, c, d, cls1)
        protos = self._class_mlp(t16, b * c)
        feat32, feat16 = self._upscale(img32, img16, b, g, fused)
        if cfg.spatial_convs:
            feat32 = self._spatial_convs(feat32, feat16, b, g)
        return self._classify(feat32, protos, cls1, ex, b, c, g)

    def _decoder_stream(self, query32: Tensor, pe32: Tensor, rows: int, hw: int, fused: bool):
        """The mask decoder's image side (``_stream_bufs``), filled from the query embeddings; the transformer updates it in place."""
        img32, img16, imgpe16 = self._stream_bufs("md.img", rows, fused)
        if fused:
            L.add_cast(query32, out32=img32, dt=L.LA_F32)
        else:
            L.add_cast(query32, out32=img32, out16=img16, dt=self.idti)
            L.add_cast(query32, pe32, hw, out16=imgpe16, dt=self.idti)
        return img32, img16, imgpe16

    def _class_mlp(self, t16: Tensor, rows: int) -> Tensor:
        """class_mlp (mask_decoder.py:290): 3 x Linear, ReLU between -> the prototypes [rows, class_width] fp32."""
        w, p, md, d = self.w32, self.p, "mask_decoder", self.cfg.embed_dim
        h1 = self.dbuf("md.cm1", (rows, d))
        L.gemm(t16, p[md + ".class_mlp.0.w"], bias=w[md + ".class_mlp.layers.0.bias"], out16=h1, act=L.ACT_RELU)
        h2 = self.dbuf("md.cm2", (rows, d))
        L.gemm(h1, p[md + ".class_mlp.1.w"], bias=w[md + ".class_mlp.layers.1.bias"], out16=h2, act=L.ACT_RELU)
        protos = self.f32("md.protos", (rows, self.cfg.class_width))
        L.gemm(h2, p[md + ".class_mlp.2.w"], bias=w[md + ".class_mlp.layers.2.bias"], out32=protos)
        return protos

    def _upscale(self, img32: Tensor, img16, b: int, g: int, fused: bool):
        """output_upscaling (mask_decoder.py:291): ConvT(k2,s2) -> LN2d -> GELU -> ConvT(k2,s2), both as pixel-shuffle GEMMs ->
        (feat32, feat16): the [B*16hw, class_width] map in fp32 and as the first spatial convolution's operand."""
        cfg, w, p, md = self.cfg, self.w32, self.p, "mask_decoder"
        hw, c1, cf = g * g, cfg.up_mid, cfg.class_width
        up1 = self.f32("md.up1", (b * 4 * hw, c1))
        if fused:       # the stream itself is the (fp32) operand: there is no separate copy to read
            L.gemm(img32, p[md + ".up0.w"], bias=w[md + ".output_upscaling.0.bias"], out32=up1, map=L.MAP_CONVT2X2, p=(g, g, c1, 0, 0))
        else:
            self.igemm(img16, md + ".up0.w", bias=w[md + ".output_upscaling.0.bias"], out32=up1, map=L.MAP_CONVT2X2, p=(g, g, c1, 0, 0))
        up1h = self.ibuf("md.up1h", b * 4 * hw, c1)
        L.layernorm(up1, w[md + ".output_upscaling.1.weight"], w[md + ".output_upscaling.1.bias"], 1e-6, gelu=True, out16=up1h, dt=self.idti)
        npix = 16 * hw
        feat32 = self.f32("md.feat32", (b * npix, cf))
        feat16 = self.f32("md.feat16f", (b * npix, cf)) if self.isplit else self.dbuf("md.feat16", (b * npix, cf))
        self.igemm(up1h, md + ".up3.w", bias=w[md + ".output_upscaling.3.bias"], out32=feat32, out16=None if self.isplit else feat16,
                   map=L.MAP_CONVT2X2, p=(2 * g, 2 * g, cf, 0, 0))
        return feat32, feat16

    def _spatial_convs(self, feat32: Tensor, feat16: Tensor, b: int, g: int) -> Tensor:
        """spatial_convs (mask_decoder.py:294-297): cfg.spatial_convs x Conv2d(3 x 3), LN2d + GELU between -> the map the pixels are
        classified on, fp32.  Three operand modes: la_conv3x3_split, la_conv3x3_f32 (both implicit GEMMs on an fp32 map), im2col + GEMM."""
        cfg, w, p, md = self.cfg, self.w32, self.p, "mask_decoder"
        cf, npix = cfg.class_width, 16 * g * g
        implicit = self.ddt == torch.float32 and cf % 32 == 0
        col = None if implicit else self.dbuf("md.col", (b * npix, 9 * cf))
        if self.isplit:       # the up3 GEMM cannot emit a second fp32 copy in split mode: the first conv reads its fp32 output
            L.add_cast(feat32, out32=feat16, dt=L.LA_F32)
        for i in range(cfg.spatial_convs):
            if implicit:      # fp32 implicit GEMM: no im2col buffer (feat16 IS fp32 here)
                nxt = self.f32("md.feat32b" if i % 2 == 0 else "md.feat32", (b * npix, cf))
                # (32 -> 32 channels, the D = 256 decoder: three fp16 products on plane pairs - fp32-class accuracy at ~3x the rate of
                # the exact-fp32 MFMA, which bounds la_conv3x3_f32; other widths keep that kernel)
                conv = L.conv3x3_split if (self.conv_split and L.conv3x3_split_ok(cf, cf)) else L.conv3x3_f32
                conv(feat16, b, 4 * g, 4 * g, cf, p[f"{md}.sc{i}.w"], w[f"{md}.spatial_convs.{3 * i}.bias"], cf, nxt)
                feat32 = nxt
            else:
                L.im2col_3x3(feat16, b, 4 * g, 4 * g, cf, col)
                L.gemm(col, p[f"{md}.sc{i}.w"], bias=w[f"{md}.spatial_convs.{3 * i}.bias"], out32=feat32)
            if i < cfg.spatial_convs - 1:
                self.dln(feat32, f"{md}.spatial_convs.{3 * i + 1}", 1e-6, gelu=True, out16=feat16)
        return feat32

    def _classify(self, feat32: Tensor, protos: Tensor, cls1: Optional[Tensor], ex, b: int, c: int, g: int) -> Tensor:
        """The classification head (mask_decoder.py:299-314, 353-362) -> low-res logits (B, C, 4g, 4g), a fresh tensor.  ex: (N, C, flags)
        of segment_example_logits; cls1: the coarse logits of classification_levels = 2."""
        cfg, w, md = self.cfg, self.w32, "mask_decoder"
        cf, npix = cfg.class_width, 16 * g * g
        if ex is not None:
            nex, ncls, fex = ex
            seg = torch.empty(b, ncls, 4 * g, 4 * g, device=self.dev, dtype=torch.float32)
            L.classify_max(feat32, protos, fex, b, npix, nex, ncls, cf, seg)
            return seg
        seg = torch.empty(b, c, 4 * g, 4 * g, device=self.dev, dtype=torch.float32)
        if cls1 is not None:            # level_reducer over [fine logits, x4 enlargement of the coarse ones] (mask_decoder.py:358-362)
            cls0 = self.f32("md.cls0", (b, c, 4 * g, 4 * g))
            L.classify(feat32, protos, b, npix, c, cf, cls0)
            L.level_reduce(cls0, cls1, w[md + ".level_reducer.weight"], w[md + ".level_reducer.bias"], b, c, g, g, seg)
            return seg
        if cfg.conv_classification:     # prototype_tconv -> one cf x 5 x 5 kernel per class, F.conv2d(padding=2) per episode (:302-307)
            k1 = self.f32("md.k1", (b * c, cf, 3, 3))
            kern = self.f32("md.kern", (b, c, 25, cf))
            L.proto_kernels(protos, w[md + ".prototype_tconv.0.weight"], w[md + ".prototype_tconv.1.weight"], b * c, cf, k1, kern)
            L.classify_conv(feat32, kern, b, c, 4 * g, 4 * g, cf, seg)
            return seg
        if cf > 64:                     # the same product over a wide map (downsample rate 1): la_classify takes widths up to 64
            L.classify_wide(protos, feat32, b, npix, c, cf, seg)
            return seg
        L.classify(feat32, protos, b, npix, c, cf, seg)
        return seg

    # ------------------------------------------------------------------------------------------------
    # post-processing (lam.py:383-453, 92-93)
    # ------------------------------------------------------------------------------------------------
    def post_sizes(self, dims: Tensor):
        """Host side of postprocess_masks: per-item (orig_h, orig_w, crop_h, crop_w) + the padded output frame."""
        cfg = self.cfg
        s = cfg.image_size
        # plain Python on the (tiny) dims list: torch CPU reductions wake the whole intra-op thread pool (measured
        # ~19 ms per call on a 128-thread host) which would dwarf the GPU time of a small episode batch
        dl = dims.detach().to("cpu").tolist()                      # [B][M+1][2]
        hmax = max(int(hw[0]) for item in dl for hw in item)
        wmax = max(int(hw[1]) for item in dl for hw in item)
        sizes = []
        for item in dl:
            oh, ow = int(item[0][0]), int(item[0][1])
            if cfg.custom_preprocess:
                sc = s * 1.0 / max(oh, ow)
                ph, pw = int(oh * sc + 0.5), int(ow * sc + 0.5)
            else:
                ph, pw = s, s
            sizes.append([oh, ow, ph, pw])
        return torch.tensor(sizes, dtype=torch.int32), hmax, wmax

    def postprocess_dev(self, seg: Tensor, sizes_d: Tensor, hmax: int, wmax: int, flag_gts_u8: Optional[Tensor], want_argmax: bool):
        """Device side (capturable): bilinear to S x S, crop + resample + pad + flag_gts (+ argmax)."""
        b, c, h, wd = seg.shape
        s = self.cfg.image_size
        big = self.f32("post.big", (b * c, s, s))
        L.bilinear(seg, b * c, h, wd, s, s, big)
        logits = torch.empty(b, c, hmax, wmax, device=self.dev, dtype=torch.float32)
        am = torch.empty(b, hmax, wmax, device=self.dev, dtype=torch.int64) if want_argmax else None
        L.post_final(big, b, c, s, sizes_d, flag_gts_u8, hmax, wmax, logits, am)
        return logits, am

    def postprocess(self, seg: Tensor, dims: Tensor, flag_gts: Optional[Tensor] = None, want_argmax: bool = False):
        sizes, hmax, wmax = self.post_sizes(dims)
        fg = self.h2d(flag_gts, torch.uint8).contiguous() if flag_gts is not None else None
        logits, am = self.postprocess_dev(seg.contiguous(), self.h2d(sizes), hmax, wmax, fg, want_argmax)
        return (logits, am) if want_argmax else logits
