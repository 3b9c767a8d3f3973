"""ctypes binding of libla_hip.so (include/la_hip.h).

The library is the product: there is NO fallback.  If the shared object is missing or a call
fails, a RuntimeError is raised (allocation failures keep the substring "out of memory" that the
reference's training loop greps for, /root/reference/label_anything/experiment/run.py:339-340).

Every entry point is stated once in SIGNATURES (``lib()`` types the loaded functions from it) and every launch goes through ``_call``,
which refuses tensors that are not on the current device before it touches the stream or the library.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libla_hip.so")      # the one product library; no environment switch (tools/_dbglib.py re-points this
#                                                     attribute for measurement builds before the first call)

LA_F16, LA_BF16, LA_F32, LA_F16X2 = 0, 1, 2, 3
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD = 0, 1, 2, 3
MAP_NONE, MAP_GROUP, MAP_WINDOW_MERGE, MAP_CONVT2X2, MAP_WINDOW_PART, MAP_CONV3X3 = 0, 1, 2, 3, 4, 5
ATTN_PLAIN, ATTN_RELPOS, ATTN_RELPOS_WIN16 = 0, 1, 2

_DT = {torch.float16: LA_F16, torch.bfloat16: LA_BF16, torch.float32: LA_F32}


class LaGemmEpilogue(C.Structure):
    _fields_ = [
        ("bias", C.c_void_p), ("res", C.c_void_p), ("ldr", C.c_int), ("res_mod", C.c_int),
        ("out32", C.c_void_p), ("ld32", C.c_int), ("out16", C.c_void_p), ("ld16", C.c_int),
        ("act", C.c_int), ("map", C.c_int),
        ("p0", C.c_int), ("p1", C.c_int), ("p2", C.c_int), ("p3", C.c_int), ("p4", C.c_int),
        ("vt", C.c_void_p), ("vt_col0", C.c_int), ("vt_T", C.c_int), ("vt_Tpad", C.c_int),
        ("vt_hd", C.c_int), ("vt_heads", C.c_int), ("vt_ws", C.c_int), ("amap", C.c_int), ("a_kmod", C.c_int), ("ksplit", C.c_int),
        ("aux16", C.c_void_p), ("ldaux", C.c_int),
        ("nstat_out", C.c_void_p), ("rvec", C.c_void_p), ("rvec_rpg", C.c_int), ("nstat_in", C.c_void_p), ("ncol", C.c_void_p),
    ]


# Every entry point include/la_hip.h declares besides la_last_error / la_version, in the header's order: its name and one letter per
# parameter - p device pointer, h host pointer (a struct, an out-parameter, an array the HOST reads), i int, l long, q long long,
# f float, s the stream (last, or absent: a host-only function).  tests/test_lib_signatures_cpu.py holds the table against the header's
# prototypes position by position.  p, h and s all travel as c_void_p (None, integers, ctypes arrays and byref(...) are taken), but only
# at a p does ``_call`` take a tensor; the scalar letters are what keeps an element count beyond 2^31 from travelling as a C int.
SIGNATURES = dict(line.split() for line in """
    la_gemm_variant                         i
    la_gemm_fused_act_ok                    iii
    la_gemm                                 pipiiiihis
    la_gemm_plan                            pipiiiihiih
    la_mfma_shape_probe                     pppiiis
    la_conv3x3_f32                          piiiippips
    la_conv3x3_split_ok                     ii
    la_conv3x3_split                        piiiippips
    la_layernorm                            ppiiippfippppiiiiis
    la_im2col_patch                         piiipis
    la_im2col_3x3                           piiiipis
    la_relpos_terms                         piiiippppis
    la_attn_fwd                             pppppppiiiiiifiis
    la_dense_pe                             piips
    la_point_embed                          pppiiippppps
    la_mask_embed                           ppiiiiihppppppis
    la_mask_embed_pooled                    ppiiiiihppppppis
    la_attn_small                           pipipiiiiiippiis
    la_colmean                              piiipps
    la_class_mean                           ppiiiips
    la_region_mean                          piiiiiips
    la_classify_max                         pppiiiiipps
    la_classify                             ppiiiips
    la_add_cast                             ppilippis
    la_nchw_to_nhwc                         piiippis
    la_nhwc_to_nchw                         piiips
    la_transpose_many                       pis
    la_bilinear                             piiiiips
    la_post_final                           piiippiipps
    la_confmat_update                       ppilpiiqppps
    la_resample_u8                          pliiippips
    la_u8_to_chw_norm                       piiiihhps
    la_prompt_masks                         ppppiiiiiiipps
    la_focal_loss                           ppiilfifqppppls
    la_logits_objective_workspace_bytes     iilh
    la_logits_objective                     ppiilqiffffipppppls
    la_prompt_contrastive_workspace_bytes   iiih
    la_prompt_contrastive                   ppiiiipppppppls
    la_adamw_step                           pppplfffffifs
    la_gemm_tn                              pipipiiiis
    la_gemm_tn_db                           pipipiiiips
    la_colsum_acc                           pilips
    la_layernorm_bwd                        pplippfippps
    la_layernorm_bwd_res                    pplippfipppipps
    la_act_fwd                              pplis
    la_act_bwd                              ppplis
    la_attn_small_lse                       pipiiiiiips
    la_attn_small_bwd                       pipipippipiiiiippps
    la_bilinear_bwd                         piiilipiilis
    la_bilinear_bwd_set_ok                  iiii
    la_bilinear_bwd_set                     piiilipiilis
    la_bilinear_rows                        piiiipiis
    la_bilinear_rows_bwd_set                piiiipiis
    la_region_mean_bwd                      piiiiiips
    la_classify_max_bwd                     ppppiiiiipps
    la_classify_bwd                         pppiiiipps
    la_row_broadcast                        pliifps
    la_twoway_pe_layout                     piips
    la_twoway_t2i                           ppppppppiiiiipps
    la_twoway_i2t                           pppppppppppfiiiiis
    la_stream_mlp_ok                        ii
    la_stream_mlp                           pppppppppfliis
    la_attn_fwd_lse                         ppppiiiiifis
    la_head_transpose                       piiiiiipis
    la_attn_bwd                             pppppppppiiiiifis
    la_attn_fwd_relpos_lse                  ppppppiiiiiifis
    la_attn_bwd_relpos                      pppppppppppppiiiiiifis
    la_relpos_bwd                           ppppppppiiiifis
    la_cast                                 pipilfs
    la_transpose16                          piiiipiips
    la_gemm_tn16                            pipipiiiiiipis
    la_axpy                                 pplfs
    la_gelu_fwd16                           pplis
    la_gelu_bwd16                           pppplis
    la_qk_fp8                               plipis
    la_attn_fwd_fp8                         pppiiiiifis
    la_colmean16                            piiiippiiiis
    la_layernorm_g                          ppiiiippfppiiipis
    la_attn_fwd_cs                          pppppppiiiiiifipiiis
    la_attn_fwd_rows                        ppppiiiiiifipiipis
    la_attn_fwd_plan                        ihh
    la_attn_bwd_plan                        ihh
    la_colsum_fold                          piiifpis
    la_add_rowvec                           ppliis
    la_add_rowvec_split                     ppliips
    la_norm_finalize                        piiifppiipis
    la_norm_stats                           piiifppis
    la_error_count                          ppiiiiipps
    la_error_points                         ppiiiiipipppliipps
    la_rle_scan                             ppipps
    la_rle_decode                           pppiiips
    la_rle_prompt_masks                     pppppppiiiiipps
    la_rle_ground_truth                     ppppppiiips
    la_rle_points                           pppppipps
    la_classify_wide                        ppiiiips
    la_classify_wide_bwd                    pppiiiipps
    la_level_reduce                         ppppiiiips
    la_level_reduce_bwd                     ppppiiiipppps
    la_proto_kernels                        pppiipps
    la_proto_kernels_bwd                    pppppiipppps
    la_classify_conv                        ppiiiiips
    la_classify_conv_bwd                    pppiiiiipps
    la_extract_pool_plan                    iiiihhh
    la_extract_pool                         ppiiiiiiipps
    la_extract_fold                         ppiiips
    la_extract_unfold                       pppiiips
    la_extract_pool_lse                     ppiiiiiiippps
    la_extract_pool_bwd_plan                iiiihhh
    la_extract_pool_bwd                     ppipppiiiiiippps
    la_extract_fold_bwd                     pppiiippps
    la_extract_unfold_bwd                   pppiiippps
    la_rope_qk                              pliiiiiippis
    la_im2col_patch_pad                     piiiipis
    la_sim_prepare                          pliiips
    la_sim_class_bits                       piiiiips
    la_sim_max_plan                         iiiiiihh
    la_sim_max                              pppiiiiipqps
""".strip().splitlines())
EXPORTS = list(SIGNATURES)                  # (tests check the .so exports all of them)
_CTYPE = {"p": C.c_void_p, "h": C.c_void_p, "s": C.c_void_p, "i": C.c_int, "l": C.c_long, "q": C.c_longlong, "f": C.c_float}
_STREAMED = frozenset(name for name, sig in SIGNATURES.items() if sig.endswith("s"))
_Tensor = torch.Tensor                      # bound once: ``_call`` asks this of every pointer argument of every launch
_DEVPTRS = {name: tuple(i for i, k in enumerate(sig) if k == "p") for name, sig in SIGNATURES.items()}      # where a tensor may stand

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"labelanything_amd: HIP extension {LIB_PATH} is missing - build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU/eager fallback)")
        l = C.CDLL(LIB_PATH)
        l.la_last_error.restype = C.c_char_p
        l.la_version.restype = C.c_int
        for name, sig in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = C.c_int, [_CTYPE[k] for k in sig]
        _lib = l
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().la_last_error().decode()
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def _dev(t: torch.Tensor) -> int:
    """Every launch goes to the CURRENT device's current stream: refuse tensors that live elsewhere instead of enqueueing a
    kernel on another GPU's stream (single-process multi-GPU hosts must wrap calls in ``torch.cuda.device(t.device)``).
    Returns the current device."""
    if not t.is_cuda:
        raise RuntimeError("labelanything_amd kernels need device tensors (no CPU fallback)")
    cur = torch.cuda.current_device()
    if t.device.index != cur:
        raise RuntimeError(f"tensor on {t.device} but the current device is cuda:{cur}: "
                           "wrap the call in `with torch.cuda.device(tensor.device)`")
    return cur


def _call(fn, *args, also=()) -> None:
    """The one path into the library: ``fn(*args[, current stream])``, the return code checked.  A tensor may stand wherever the
    signature has a device pointer and travels as its address; None, plain integers (addresses included) and ctypes objects go to ctypes
    as they are.  Every tensor - among ``args`` or ``also``, the tensors a call reaches through a struct or a pointer list - must be on
    the current device (``_dev``, which runs once a call: the tensors after the first are compared with the device it returned).  All of
    that happens before the stream is fetched and the library entered: a refused call touches neither."""
    name, argv, cur = fn.__name__, list(args), None
    for i in _DEVPTRS[name]:
        a = argv[i]
        if isinstance(a, _Tensor):
            if a.get_device() != cur:           # -1 for a host tensor
                cur = _dev(a)
            argv[i] = a.data_ptr()
    for a in also:
        if isinstance(a, _Tensor) and a.get_device() != cur:
            cur = _dev(a)
    if name in _STREAMED:
        argv.append(torch.cuda.current_stream().cuda_stream)
    rc = fn(*argv)
    if rc != 0:
        _check(rc, name)


GEMM_VARIANT_MFMA32 = 0x10000


def gemm_variant(v: int = -1) -> int:
    """la_gemm_variant: the persistent kernel of the single-plane shapes with K % 64 == 0, K >= 128 (``gemm_plan`` says which calls those
    are) - 2 (default): gemm_t256w, four waves x 512 registers (gemm_w4.hip); 1: gemm_t256q, eight waves in quadrant phases; 0:
    gemm_t256p, the BK 32 kernel, which two-plane shapes take at every value.  The LaGemmEpilogue.aux16 / nstat_* forms exist at 2 only.
    + GEMM_VARIANT_MFMA32: gemm_t256w keeps the 32x32x16 MFMA where the plan (``LaGemmPlan.mfma``) would take 16x16x32.
    All are bit-identical; v < 0 only queries.  Returns the previous value."""
    return int(lib().la_gemm_variant(int(v)))


def dt_of(t: torch.Tensor) -> int:
    return _DT[t.dtype]


# ----------------------------------------------------------------------------------------------
class LaGemmPlan(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("kernel", "epi", "planes", "direct", "ragged", "gm", "ksplit", "kchunk", "grid", "block", "lds_bytes", "mfma")]


GEMM_KERNELS = ("NT", "DMA128", "DMA256x128", "T256", "T256P", "T256Q", "T256W", "F32_N32", "F32_N128", "F32_SMALL", "SKINNY")   # LaGemmPlan.kernel


def _addr(x) -> Optional[int]:
    """Device address of a tensor; None and plain integers (a planned call needs no memory) pass through."""
    return x.data_ptr() if isinstance(x, torch.Tensor) else x


def _gemm_epilogue(m: int, n: int, *, bias=None, res=None, res_mod=0, out32=None, out16=None, act=ACT_NONE, map=MAP_NONE, p=(0, 0, 0, 0, 0), vt=None,
                   vt_col0=0, vt_T=0, vt_Tpad=0, vt_hd=64, vt_heads=0, vt_ws=0, amap=MAP_NONE, a_kmod=0, ksplit=0, aux16=None, nstat_out=None, rvec=None,
                   rvec_rpg=0, nstat_in=None, ncol=None, ldr=None, ld32=None, ld16=None, ldaux=None) -> LaGemmEpilogue:
    """The LaGemmEpilogue of a ``gemm`` / ``gemm_plan`` call.  Buffers are tensors or plain addresses; the leading dimension of a tensor
    is its row stride, of an address the ld* argument (default: n)."""
    def ld(x, given):
        if x is None:
            return 0
        if given is not None:
            return given
        return n if not isinstance(x, torch.Tensor) else (x.stride(-2) if x.dim() >= 2 else 0)

    e = LaGemmEpilogue()
    e.bias, e.res, e.out32, e.out16, e.vt, e.aux16 = _addr(bias), _addr(res), _addr(out32), _addr(out16), _addr(vt), _addr(aux16)
    e.ldr, e.ld32, e.ld16, e.ldaux = ld(res, ldr), ld(out32, ld32), ld(out16, ld16), ld(aux16, ldaux)
    e.res_mod = res_mod
    e.act, e.map = act, map
    e.p0, e.p1, e.p2, e.p3, e.p4 = p
    e.vt_col0, e.vt_T, e.vt_Tpad, e.vt_hd, e.vt_heads = vt_col0, vt_T, vt_Tpad, vt_hd, vt_heads
    e.vt_ws = vt_ws
    e.amap = amap
    e.a_kmod = a_kmod
    e.ksplit = ksplit
    mpad = -(-m // 256) * 256
    if isinstance(nstat_out, torch.Tensor) and (nstat_out.dtype != torch.float32 or nstat_out.numel() < m * (n // 64) * 2):
        raise RuntimeError(f"gemm: nstat_out must be fp32 with at least M * (N / 64) * 2 = {m * (n // 64) * 2} entries")
    if isinstance(nstat_in, torch.Tensor) and (nstat_in.dtype != torch.float32 or nstat_in.numel() < mpad * 2 or ncol is None
                                               or ncol.dtype != torch.float32 or ncol.numel() < n):
        raise RuntimeError(f"gemm: nstat_in must be fp32 [ceil(M / 256) * 256, 2] (>= {mpad * 2} entries) and needs ncol fp32 [N]")
    if isinstance(rvec, torch.Tensor) and (rvec.dtype != torch.float32 or rvec_rpg <= 0 or rvec.numel() < -(-m // rvec_rpg) * n):
        raise RuntimeError("gemm: rvec must be fp32 [ceil(M / rvec_rpg), N] with rvec_rpg > 0")
    e.nstat_out, e.rvec, e.nstat_in, e.ncol = _addr(nstat_out), _addr(rvec), _addr(nstat_in), _addr(ncol)
    e.rvec_rpg = rvec_rpg
    return e


def gemm(a: torch.Tensor, w: torch.Tensor, *, M=None, lda=None, **epilogue) -> None:
    """C = epilogue(a @ w.T).  a: [M,K] 16-bit (row stride lda), w: [N,K] 16-bit.  a_kmod > 0: w is [N, j*a_kmod] (split-precision
    planes [W_hi | W_lo]) and the columns of a repeat with period a_kmod.  aux16 (training, shapes with ``gemm_fused_act_ok``): with
    ACT_GELU the pre-activation is written there beside out16 = GELU; with ACT_GELU_BWD out16 = (a @ w.T) * gelu'(aux16).
    nstat_out / rvec / nstat_in / ncol: the producer and consumer sides of a LayerNorm folded into its neighbour GEMMs (see
    LaGemmEpilogue in include/la_hip.h; ``norm_finalize`` turns the producer's partial sums into the consumer's (mean, rstd) rows).
    The epilogue keywords are those of ``_gemm_epilogue``."""
    m = a.shape[0] if M is None else M
    k = w.shape[1]
    n = w.shape[0]
    e = _gemm_epilogue(m, n, **epilogue)
    _call(lib().la_gemm, a, a.stride(0) if lda is None else lda, w, w.stride(0), m, n, k, C.byref(e), dt_of(a), also=epilogue.values())


def gemm_plan(a, lda: int, w, ldw: int, m: int, n: int, k: int, dt: int, ncu: int = 0, **epilogue) -> LaGemmPlan:
    """la_gemm_plan: what ``gemm`` would launch for these arguments (kernel family - GEMM_KERNELS[plan.kernel] -, epilogue, grid), with
    la_gemm's argument errors and no launch.  a, w and the epilogue buffers are tensors or plain integer addresses (they are only tested
    for None and alignment), so this runs without a GPU when ncu is given; ncu <= 0 takes the CU count of the current device."""
    plan = LaGemmPlan()
    e = _gemm_epilogue(m, n, **epilogue)
    _call(lib().la_gemm_plan, _addr(a), lda, _addr(w), ldw, m, n, k, C.byref(e), dt, ncu, C.byref(plan))
    return plan


_ATTN_CALL_PTRS = ("qkv", "vt", "out16", "relh", "relw", "tabh", "tabw", "lse", "cspart", "padrow", "dout16", "dvec", "dqkv", "drelh", "drelw", "dtabh",
                   "dtabw")
_ATTN_CALL_INTS = ("B", "heads", "T", "Tpad", "G", "E", "mode", "csH", "csW", "imgH", "imgW", "dt")


class LaAttnCall(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in _ATTN_CALL_PTRS] + [(f, C.c_int) for f in _ATTN_CALL_INTS]


class LaAttnLaunch(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("kernel", "mode", "nh", "vrow", "grid", "block", "lds_bytes")]


class LaAttnPlan(C.Structure):
    _fields_ = [("launch", LaAttnLaunch * 2), ("n", C.c_int), ("repeat", C.c_int), ("ry", C.c_int)]


# LaAttnPlan entry points (LA_ATTN_EP_*), kernel families (LA_ATTN_K_*) and the bias forms of csrc/attn_plan.h (LaAttnLaunch.mode)
ATTN_ENTRIES = ("attn_fwd", "attn_fwd_rows", "attn_fwd_lse", "attn_fwd_relpos_lse", "attn_bwd", "attn_bwd_relpos", "relpos_bwd")
ATTN_KERNELS = ("FWD", "WINDOW", "BWD_DQ", "BWD_DKV", "RELPOS_BWD_ROWS", "RELPOS_BWD")
ATTN_FWD_MODES = ("NOBIAS", "TERMS", "TERMS_ROW64", "TABLES_WIN", "TABLES_ROW64", "TABLES_WIN16")
ATTN_BWD_MODES = ("NOBIAS", "TERMS", "ROW64", "WIN16")
ATTN_DKV_MODES = ("NOBIAS", "TERMS", "STAGED")


def _attn_plan(fn, entry: str, **call) -> LaAttnPlan:
    c, plan = LaAttnCall(), LaAttnPlan()
    for k, v in call.items():
        setattr(c, k, _addr(v))
    _call(fn, ATTN_ENTRIES.index(entry), C.byref(c), C.byref(plan))
    return plan


def attn_fwd_plan(entry: str, **call) -> LaAttnPlan:
    """la_attn_fwd_plan: what the forward entry point ``entry`` (``attn_fwd`` - also ``attn_fwd_cs`` -, ``attn_fwd_rows``, ``attn_fwd_lse``,
    ``attn_fwd_relpos_lse``) would launch for the LaAttnCall fields given as keywords (B, heads, T, Tpad, G, E, mode, dt, buffers, ...;
    the rest zero), with its argument errors and no launch.  Buffers are tensors or plain integer addresses - only tested for None -, so
    this runs without a GPU."""
    return _attn_plan(lib().la_attn_fwd_plan, entry, **call)


def attn_bwd_plan(entry: str, **call) -> LaAttnPlan:
    """la_attn_bwd_plan: the same for ``attn_bwd``, ``attn_bwd_relpos`` (two launches: dq, then dk / dv) and ``relpos_bwd`` (one launch,
    ``plan.repeat`` times)."""
    return _attn_plan(lib().la_attn_bwd_plan, entry, **call)


def mfma_shape_probe(a: torch.Tensor, w: torch.Tensor, shape: int) -> torch.Tensor:
    """la_mfma_shape_probe: a [32, K] . w [32, K]^T (16-bit, K % 64 == 0) on one wave with MFMA shape 0 (32x32x16) or 1 (16x16x32),
    fp32 [32, 32]: the accumulators as they are, K ascending in 64-deep tiles."""
    if a.dtype != w.dtype or a.shape != w.shape or a.shape[0] != 32 or not (a.is_contiguous() and w.is_contiguous()):
        raise RuntimeError("mfma_shape_probe: a and w must be contiguous [32, K] of one 16-bit type")
    out = torch.empty(32, 32, device=a.device, dtype=torch.float32)
    _call(lib().la_mfma_shape_probe, a, w, out, a.shape[1], dt_of(a), shape)
    return out


def norm_finalize(part: Optional[torch.Tensor], m: int, e: int, eps: float, mr: torch.Tensor, x16: Optional[torch.Tensor] = None, rpg: int = 0,
                  cs_part: Optional[torch.Tensor] = None) -> None:
    """mr[row] = (mean, rstd) from a producer GEMM's partial row sums ``part`` ([m, e / 64, 2]; None: mr is an input); cs_part (with x16,
    rpg): column sums of rstd (x16 - mean) per 128-row chunk of every group of rpg rows (``norm_cs_chunks(rpg)`` chunks per group)."""
    mpad = -(-m // 256) * 256
    if mr.dtype != torch.float32 or mr.numel() < mpad * 2 or not mr.is_contiguous():
        raise RuntimeError(f"norm_finalize: mr must be contiguous fp32 with >= {mpad * 2} entries")
    if part is not None and (part.dtype != torch.float32 or part.numel() < m * (e // 64) * 2):
        raise RuntimeError("norm_finalize: part must be fp32 [m, e / 64, 2]")
    if cs_part is not None:
        if x16 is None or rpg <= 0 or m % rpg or x16.shape[0] < m or x16.shape[1] != e or x16.stride(1) != 1:
            raise RuntimeError("norm_finalize: column sums need x16 [m, e] and m % rpg == 0")
        if cs_part.dtype != torch.float32 or cs_part.numel() < (m // rpg) * norm_cs_chunks(rpg) * e:
            raise RuntimeError("norm_finalize: cs_part too small")
    _call(lib().la_norm_finalize, part, m, e // 64, e, eps, mr, x16, x16.stride(0) if x16 is not None else 0, rpg, cs_part,
          dt_of(x16) if x16 is not None else LA_F16)


def norm_cs_chunks(rpg: int) -> int:
    """Column-sum partials per group that ``norm_finalize(cs_part=...)`` writes (128 rows each)."""
    return -(-rpg // 128)


def norm_stats(x: torch.Tensor, eps: float, x16: torch.Tensor, mr: torch.Tensor) -> None:
    """x16 = 16-bit rounding of the fp32 rows x, mr[row] = (mean, rstd): the entry of a folded-LayerNorm block stack."""
    m, e = x.shape
    mpad = -(-m // 256) * 256
    if x.dtype != torch.float32 or x.stride(1) != 1 or x16.shape != x.shape or not x16.is_contiguous() or mr.dtype != torch.float32 \
            or mr.numel() < mpad * 2:
        raise RuntimeError("norm_stats: x fp32 [m, e], x16 contiguous 16-bit [m, e], mr fp32 with >= ceil(m / 256) * 256 * 2 entries")
    _call(lib().la_norm_stats, x, x.stride(0), m, e, eps, x16, mr, dt_of(x16))


def gemm_fused_act_ok(m: int, n: int, k: int) -> bool:
    """True when ``gemm(..., aux16=...)`` runs for this shape (the persistent four-wave kernel's direct epilogue)."""
    return bool(lib().la_gemm_fused_act_ok(m, n, k))


def layernorm(x: torch.Tensor, gamma, beta, eps: float, *, x2=None, gelu=False, out32=None, out16=None,
              out16_pe=None, pe=None, pe_mod=0, window=0, H=0, W=0, dt=LA_F16) -> None:
    rows, e = x.shape[0], x.shape[1]
    if x2 is not None and (x2.shape[1] != e or x2.stride(1) != 1 or x2.stride(0) != x.stride(0)):
        # the kernel walks x and x2 with ONE row stride: a contiguous x2 beside a column slice x would be read at the wrong rows
        raise RuntimeError(f"layernorm: x2 must have the row stride of x ({x.stride(0)}), got {x2.stride(0)}")
    if window < 0:
        # padded-map forms (LA_MAP_CONV3X3 operand layout): -1 writes the 16-bit output into the interior of [B, H + 2, W + 2] maps, -2 reads
        # the input rows from that layout; ``rows`` counts the UN-padded pixels either way
        o = out32 if out32 is not None else out16
        if window == -2:
            rows = o.shape[0]
            if x.shape[0] < (rows // (H * W)) * (H + 2) * (W + 2):
                raise RuntimeError("layernorm(window=-2): x must hold the padded maps [B * (H + 2) * (W + 2), E]")
        elif out16 is None or out16.shape[0] < (rows // (H * W)) * (H + 2) * (W + 2):
            raise RuntimeError("layernorm(window=-1): out16 must hold the padded maps [B * (H + 2) * (W + 2), ...]")
    _call(lib().la_layernorm, x, x2, x.stride(0), rows, e, gamma, beta, eps, int(gelu), out32, out16, out16_pe, pe, pe_mod, window, H, W, dt)


def im2col_patch(img: torch.Tensor, patch: int, out16: torch.Tensor, split: bool = False) -> None:
    """split: out16 is fp16 [rows, 2 K] = [hi | lo] plane pairs (LA_F16X2)."""
    bn, _, s, _ = img.shape
    dt = LA_F16X2 if split else dt_of(out16)
    if split and out16.dtype != torch.float16:
        raise RuntimeError("im2col_patch(split=True) writes fp16 plane pairs")
    _call(lib().la_im2col_patch, img, bn, s, patch, out16, dt)


def im2col_patch_pad(img: torch.Tensor, patch: int, kp: int, out: torch.Tensor, split: bool = False) -> None:
    """im2col_patch for even patch sides that are no multiple of 8: out [Bn g g, kp] (split: fp16 [Bn g g, 2 kp] = [hi | lo]), the columns
    3 patch^2 .. kp zero.  Everything the library would refuse is refused here, before it is entered."""
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3] or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError("im2col_patch_pad: img must be a contiguous fp32 [Bn, 3, S, S] tensor")
    bn, _, s, _ = img.shape
    k = 3 * patch * patch
    if patch < 2 or patch % 2 or s % patch:
        raise ValueError(f"im2col_patch_pad: patch={patch} must be even, >= 2 and divide the image side {s}")
    if kp % 64 or kp < k or kp < 128:
        raise ValueError(f"im2col_patch_pad: kp={kp} must be a multiple of 64, >= 128 and >= 3 patch^2 = {k}")
    rows = bn * (s // patch) ** 2
    if split and out.dtype != torch.float16:
        raise ValueError("im2col_patch_pad(split=True) writes fp16 plane pairs")
    if out.dtype not in _DT or tuple(out.shape) != (rows, 2 * kp if split else kp) or not out.is_contiguous():
        raise ValueError(f"im2col_patch_pad: out must be a contiguous fp16 / bf16 / fp32 [{rows}, {2 * kp if split else kp}] matrix, got "
                         f"{out.dtype} {tuple(out.shape)}")
    _call(lib().la_im2col_patch_pad, img, bn, s, patch, kp, out, LA_F16X2 if split else dt_of(out))


def im2col_3x3(x16: torch.Tensor, b: int, h: int, w: int, c: int, out16: torch.Tensor, split: bool = False) -> None:
    """split: x16 rows are fp16 plane pairs [hi (c) | lo (c)], out16 rows [9 taps of hi | 9 taps of lo] (LA_F16X2)."""
    _call(lib().la_im2col_3x3, x16, b, h, w, c, out16, LA_F16X2 if split else dt_of(x16))


def relpos_terms(qkv: torch.Tensor, b: int, heads: int, g: int, e: int, tabh, tabw, relh, relw) -> None:
    _call(lib().la_relpos_terms, qkv, b, heads, g, e, tabh, tabw, relh, relw, dt_of(qkv))


def attn_fwd(qkv, vt, out16, relh, relw, b: int, heads: int, t: int, tpad: int, g: int, e: int, scale: float, mode: int,
             tabh=None, tabw=None) -> None:
    _call(lib().la_attn_fwd, qkv, vt, out16, relh, relw, tabh, tabw, b, heads, t, tpad, g, e, scale, mode, dt_of(qkv))


# ---- decoder side ---------------------------------------------------------------------------------
def dense_pe(gauss: torch.Tensor, g: int, d: int, out: torch.Tensor) -> None:
    _call(lib().la_dense_pe, gauss, g, d, out)


def point_embed(xy, kind, shift, d: int, image_size: int, gauss, type_emb, not_a_point, no_sparse, out32) -> None:
    _call(lib().la_point_embed, xy, kind, shift, kind.numel(), d, image_size, gauss, type_emb, not_a_point, no_sparse, out32)


def _mask_embed(fn, masks, flags, n, c, hm, g, d, wlist, support, class_enc, pe, src32, src16, srcpe16, dt) -> None:
    arr = (C.c_void_p * 12)(*[w.data_ptr() for w in wlist])
    _call(fn, masks, flags, n, c, hm, g, d, arr, support, class_enc, pe, src32, src16, srcpe16, dt, also=wlist)


def mask_embed(masks, flags, p: int, c: int, hm: int, g: int, d: int, wlist, support, class_enc, pe, src32, src16, srcpe16,
               dt: int) -> None:
    _mask_embed(lib().la_mask_embed, masks, flags, p, c, hm, g, d, wlist, support, class_enc, pe, src32, src16, srcpe16, dt)


def mask_embed_pooled(masks, flags, s: int, c: int, hm: int, g: int, d: int, wlist, support, class_enc, pe, src32, src16, srcpe16,
                      dt: int) -> None:
    """la_mask_embed_pooled: one [g*g, D] slab per support image, the dense prompts of its ``c`` classes summed (TokenPool)."""
    _mask_embed(lib().la_mask_embed_pooled, masks, flags, s, c, hm, g, d, wlist, support, class_enc, pe, src32, src16, srcpe16, dt)


def attn_small(q, k, v, b: int, nq: int, nk: int, heads: int, hd: int, *, out16=None, out32=None, dt: int = LA_F16) -> None:
    """q/k/v: fp32 2-D views [rows, ld] (row stride = ld, head h at column h*hd).  dt = LA_F16X2: out16 is [rows, 2 * heads * hd]
    ([hi | lo] planes)."""
    if dt == LA_F16X2:
        out32, ldo = None, heads * hd
    else:
        ldo = (out16 if out16 is not None else out32).stride(0)
    _call(lib().la_attn_small, q, q.stride(0), k, k.stride(0), v, v.stride(0), b, nq, nk, heads, hd, out16, out32, ldo, dt)


COLMEAN_SPLIT = 16


def colmean(x, p: int, hw: int, d: int, out, scratch) -> None:
    """scratch: fp32 [p, COLMEAN_SPLIT, d]."""
    _call(lib().la_colmean, x, p, hw, d, out, scratch)


def class_mean(emb, flags_u8, b: int, m: int, c: int, d: int, out) -> None:
    _call(lib().la_class_mean, emb, flags_u8, b, m, c, d, out)


def classify(feat, protos, b: int, npix: int, c: int, cf: int, seg) -> None:
    _call(lib().la_classify, feat, protos, b, npix, c, cf, seg)


def region_mean(x, b: int, m: int, c: int, g: int, k: int, d: int, out) -> None:
    """x fp32 [b*m*c, g*g, d] -> out fp32 [b, m*k*k, c, d]: adaptive k x k average pooling of every slab, example index m*k*k + i*k + j."""
    _f32c(x, out)
    if x.numel() != b * m * c * g * g * d or out.numel() != b * m * k * k * c * d:
        raise ValueError(f"region_mean: x must hold [{b * m * c}, {g * g}, {d}] and out [{b}, {m * k * k}, {c}, {d}] elements "
                         f"(got {x.numel()} and {out.numel()})")
    _call(lib().la_region_mean, x, b, m, c, g, k, d, out)


def _classify_max_args(feat, protos, b: int, npix: int, n: int, c: int, cf: int, planes) -> None:
    _f32c(feat, protos)
    if feat.numel() != b * npix * cf or protos.numel() != b * n * c * cf:
        raise ValueError(f"classify_max: feat must hold [{b}, {npix}, {cf}] and protos [{b}, {n}, {c}, {cf}] elements")
    for t, dtype in planes:
        if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.numel() != b * c * npix):
            raise ValueError(f"classify_max: contiguous {dtype} [{b}, {c}, {npix}] planes expected")


def classify_max(feat, protos, flags_u8, b: int, npix: int, n: int, c: int, cf: int, seg, win=None) -> None:
    """seg[b, c, pix] = max over the examples n with flags_u8[b, n, c] != 0 of protos[b, n, c] . feat[b, pix]; win (int32, optional): the
    winning n (the lowest among equals), -1 where seg is -inf because no example is valid."""
    _classify_max_args(feat, protos, b, npix, n, c, cf, ((seg, torch.float32), (win, torch.int32)))
    if flags_u8.dtype != torch.uint8 or not flags_u8.is_contiguous() or flags_u8.numel() != b * n * c:
        raise ValueError(f"classify_max: flags must be contiguous uint8 [{b}, {n}, {c}]")
    _call(lib().la_classify_max, feat, protos, flags_u8, b, npix, n, c, cf, seg, win)


def add_cast(x, y=None, ymod: int = 0, *, out32=None, out16=None, dt: int = LA_F16) -> None:
    _call(lib().la_add_cast, x, y, ymod, x.shape[0], x.shape[1], out32, out16, dt)


def nchw_to_nhwc(x, n: int, c: int, hw: int, *, out32=None, out16=None, dt: int = LA_F16) -> None:
    _call(lib().la_nchw_to_nhwc, x, n, c, hw, out32, out16, dt)


def nhwc_to_nchw(x, n: int, c: int, hw: int, out) -> None:
    _call(lib().la_nhwc_to_nchw, x, n, c, hw, out)


def bilinear(x, n: int, h: int, w: int, oh: int, ow: int, out) -> None:
    _call(lib().la_bilinear, x, n, h, w, oh, ow, out)


def error_count(logits, gt, b: int, c: int, h: int, w: int, ignore_index: int, counts, preds=None) -> None:
    _call(lib().la_error_count, logits, gt, b, c, h, w, ignore_index, counts, preds)


def error_points(logits, gt, b: int, c: int, h: int, w: int, ignore_index: int, counts, num_points: int, ranks, u, dims, dims_stride: int,
                 long_side: int, custom_preprocess: bool, points, labels) -> None:
    _call(lib().la_error_points, logits, gt, b, c, h, w, ignore_index, counts, num_points, ranks, u, dims, dims_stride, long_side,
          1 if custom_preprocess else 0, points, labels)


def post_final(big, b: int, c: int, s: int, sizes_i32, flag_gts_u8, hmax: int, wmax: int, logits, argmax) -> None:
    _call(lib().la_post_final, big, b, c, s, sizes_i32, flag_gts_u8, hmax, wmax, logits, argmax)


def confmat_update(pred_i64, gt_i64, lut_i32, k: int, ignore_index: int, confmat_u64, confbin_u64, counters_u64) -> None:
    """pred / gt int64 [B, ...]; lut int32 [B, L] or None; the three accumulators are int64 tensors (bit patterns of u64)."""
    if pred_i64.dtype != torch.int64 or gt_i64.dtype != torch.int64 or pred_i64.shape != gt_i64.shape:
        raise ValueError("confmat_update: pred and gt must be int64 tensors of the same shape")
    if not (pred_i64.is_contiguous() and gt_i64.is_contiguous()):
        raise ValueError("confmat_update: label maps must be contiguous")
    b = pred_i64.shape[0]
    hw = pred_i64.numel() // b
    ell = 0
    if lut_i32 is not None:
        if lut_i32.dtype != torch.int32 or lut_i32.dim() != 2 or lut_i32.shape[0] != b or not lut_i32.is_contiguous():
            raise ValueError("confmat_update: lut must be a contiguous int32 [B, L] tensor")
        ell = lut_i32.shape[1]
    _call(lib().la_confmat_update, pred_i64, gt_i64, b, hw, lut_i32, ell, k, ignore_index, confmat_u64, confbin_u64, counters_u64)


def resample_u8(inp, n_outer: int, in_size: int, inner: int, out_size: int, bounds_i32, kk_i32, out) -> None:
    _call(lib().la_resample_u8, inp, n_outer, in_size, inner, out_size, bounds_i32, kk_i32, kk_i32.shape[1], out)


def prompt_masks(masks_u8, first_i32, count_i32, index_i32, p: int, h: int, w: int, nh: int, nw: int, s: int, mo: int, out, flags_u8) -> None:
    _call(lib().la_prompt_masks, masks_u8, first_i32, count_i32, index_i32, p, h, w, nh, nw, s, mo, out, flags_u8)


# ---- run-length annotations (rle.hip): all int32 device tensors, laid out by labelanything_amd.annotations.pack_rles -------------------
def rle_scan(runs_i32, meta_i32, k: int, ends_i32, area_i32) -> None:
    _call(lib().la_rle_scan, runs_i32, meta_i32, k, ends_i32, area_i32)


def rle_decode(ends_i32, meta_i32, sel_i32, k: int, h: int, w: int, out_u8) -> None:
    _call(lib().la_rle_decode, ends_i32, meta_i32, sel_i32, k, h, w, out_u8)


def rle_prompt_masks(ends_i32, meta_i32, first_i32, count_i32, index_i32, img_hw_i32, new_hw_i32, n: int, c: int, custom: bool, s: int, mo: int,
                     out, flags_u8) -> None:
    _call(lib().la_rle_prompt_masks, ends_i32, meta_i32, first_i32, count_i32, index_i32, img_hw_i32, new_hw_i32, n, c, 1 if custom else 0, s, mo,
          out, flags_u8)


def rle_ground_truth(ends_i32, meta_i32, first_i32, count_i32, index_i32, img_hw_i32, n: int, hmax: int, wmax: int, out_i64) -> None:
    _call(lib().la_rle_ground_truth, ends_i32, meta_i32, first_i32, count_i32, index_i32, img_hw_i32, n, hmax, wmax, out_i64)


def rle_points(ends_i32, meta_i32, area_i32, new_hw_i32, draws_i32, d: int, points, flags_u8) -> None:
    _call(lib().la_rle_points, ends_i32, meta_i32, area_i32, new_hw_i32, draws_i32, d, points, flags_u8)


def focal_loss(logits, target_i64, gamma: float, class_weighting: bool, scale: float, ignore_index: int, loss, dlogits, class_weights,
               scratch) -> None:
    b, c = logits.shape[0], logits.shape[1]
    hw = logits.numel() // (b * c)
    _call(lib().la_focal_loss, logits, target_i64, b, c, hw, gamma, int(class_weighting), scale, ignore_index, loss, dlogits, class_weights,
          scratch, scratch.numel() * scratch.element_size())


def _workspace_bytes(fn, *sizes: int) -> int:
    n = C.c_long(0)
    _call(fn, *sizes, C.byref(n))
    return int(n.value)


def logits_objective_workspace_bytes(b: int, c: int, hw: int) -> int:
    return _workspace_bytes(lib().la_logits_objective_workspace_bytes, b, c, hw)


def logits_objective(logits, target_i64, ignore_index: int, mask: int, w_focal: float, gamma: float, w_dice: float, w_fp: float,
                     class_weighting: bool, value, components, dlogits, class_weights, workspace) -> None:
    b, c = logits.shape[0], logits.shape[1]
    hw = logits.numel() // (b * c)
    _call(lib().la_logits_objective, logits, target_i64, b, c, hw, ignore_index, mask, w_focal, gamma, w_dice, w_fp, int(class_weighting),
          value, components, dlogits, class_weights, workspace, workspace.numel() * workspace.element_size())


def prompt_contrastive_workspace_bytes(b: int, n: int, d: int) -> int:
    return _workspace_bytes(lib().la_prompt_contrastive_workspace_bytes, b, n, d)


def prompt_contrastive(emb, flags_u8, c: int, t_prime, bias, loss, demb, dt_prime, dbias, workspace) -> None:
    b, n, d = emb.shape
    _call(lib().la_prompt_contrastive, emb, flags_u8, b, n, c, d, t_prime, bias, loss, demb, dt_prime, dbias, workspace,
          workspace.numel() * workspace.element_size())


def adamw_step(params, grads, exp_avg, exp_avg_sq, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
               grad_scale: float = 1.0) -> None:
    for t in (params, grads, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params.numel():
            raise ValueError("adamw_step: flat contiguous fp32 buffers of equal length expected")
    _call(lib().la_adamw_step, params, grads, exp_avg, exp_avg_sq, params.numel(), lr, beta1, beta2, eps, weight_decay, step, grad_scale)


def u8_to_chw_norm(inp, h: int, w: int, sh: int, sw: int, mean, std, out) -> None:
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    _call(lib().la_u8_to_chw_norm, inp, h, w, sh, sw, m3, s3, out)


def conv3x3_f32(x32, b: int, h: int, w: int, cin: int, wt, bias, cout: int, out32) -> None:
    _call(lib().la_conv3x3_f32, x32, b, h, w, cin, wt, bias, cout, out32)


def conv3x3_split_ok(cin: int, cout: int) -> bool:
    return bool(lib().la_conv3x3_split_ok(cin, cout))


def conv3x3_split(x32, b: int, h: int, w: int, cin: int, wt, bias, cout: int, out32) -> None:
    """la_conv3x3_f32's convolution for 32 -> 32 channels as three fp16 MFMA products on plane pairs (fp32-class accuracy, ~3x the rate)."""
    for t_, n_ in ((x32, b * h * w * cin), (wt, cout * 9 * cin), (out32, b * h * w * cout)):
        if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() < n_:
            raise RuntimeError("conv3x3_split: contiguous fp32 input [b*h*w, cin], weight [cout, 9*cin], output [b*h*w, cout]")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < cout):
        raise RuntimeError("conv3x3_split: bias must be fp32 [cout]")
    _call(lib().la_conv3x3_split, x32, b, h, w, cin, wt, bias, cout, out32)


# ---- backward kernels (training step, csrc/train.hip) ------------------------------------------------------------------------
def _f32c(*ts) -> None:
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("contiguous fp32 device tensors expected")


def _f32rows(t: torch.Tensor) -> None:
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("fp32 device matrices with unit column stride expected")


def gemm_tn(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor] = None) -> None:
    """dw[N,K] += dy[M,N]^T @ x[M,K] (and db[N] += dy.sum(0) when db is given).  dy / x may be column slices of wider matrices (row
    stride = the parent's width)."""
    _f32rows(dy), _f32rows(x), _f32c(dw)
    m, n = dy.shape
    k = x.shape[1]
    if db is not None:
        _f32c(db)
        if db.numel() != n:
            raise ValueError("gemm_tn: db must hold N elements")
    _call(lib().la_gemm_tn_db, dy, dy.stride(0), x, x.stride(0), dw, k, m, n, k, db)


def gemm_tn16(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor] = None, gsize: int = 0, gstride: int = 0) -> None:
    """dw[N,K] += dy[R,N]^T @ x[R,K] from row-major 16-bit operands (column slices allowed), db[N] += dy.sum(0); 16-bit MFMA, no
    transposed copies.  gsize / gstride: output row n -> dw row (n // gsize) * gstride + n % gsize (dw = the first row's tensor)."""
    if dy.dtype not in (torch.float16, torch.bfloat16) or x.dtype != dy.dtype:
        raise TypeError("gemm_tn16: 16-bit operands of one dtype")
    if dy.stride(1) != 1 or x.stride(1) != 1 or dy.shape[0] != x.shape[0]:
        raise ValueError("gemm_tn16: row-major operands with the same number of rows")
    _f32c(dw)
    r, n = dy.shape
    k = x.shape[1]
    if db is not None:
        _f32c(db)
        if db.numel() != n:
            raise ValueError("gemm_tn16: db must hold N elements")
    _call(lib().la_gemm_tn16, dy, dy.stride(0), x, x.stride(0), dw, k, r, n, k, gsize, gstride, db, dt_of(dy))


def colsum_acc(dy: torch.Tensor, out: torch.Tensor) -> None:
    """out[N] += dy[M,N].sum(0) (dy may be a column slice of a wider matrix)."""
    _f32rows(dy), _f32c(out)
    m, n = dy.shape
    _call(lib().la_colsum_acc, dy, dy.stride(0), m, n, out)


def layernorm_bwd(x, dy, gamma, beta, eps: float, gelu: bool, dx, dgamma, dbeta) -> None:
    _f32c(x, dy, gamma, beta, dx, dgamma, dbeta)
    rows, e = x.shape
    _call(lib().la_layernorm_bwd, x, dy, rows, e, gamma, beta, eps, int(gelu), dx, dgamma, dbeta)


def layernorm_bwd_res(x, dy, gamma, beta, eps: float, add, dx, out16, dgamma, dbeta) -> None:
    """dx = LayerNorm backward(x, dy) + add (add may be dx), optionally with a 16-bit copy of dx in out16."""
    _f32c(x, dy, gamma, beta, dx, dgamma, dbeta, add)
    rows, e = x.shape
    _call(lib().la_layernorm_bwd_res, x, dy, rows, e, gamma, beta, eps, 0, add, dx, out16, dt_of(out16) if out16 is not None else LA_F16,
          dgamma, dbeta)


def transpose_many(tile_table: torch.Tensor) -> None:
    """tile_table: int64 [ntiles, 4] on the device - (src, dst, rows << 32 | cols, r0 << 32 | c0) per 32 x 32 tile; dst[c][r] = src[r][c]."""
    if tile_table.dtype != torch.int64 or tile_table.dim() != 2 or tile_table.shape[1] != 4 or not tile_table.is_contiguous():
        raise ValueError("transpose_many needs a contiguous int64 [ntiles, 4] table")
    _call(lib().la_transpose_many, tile_table, tile_table.shape[0])


def act_fwd(x, y, kind: int) -> None:
    _f32c(x, y)
    _call(lib().la_act_fwd, x, y, x.numel(), kind)


def act_bwd(x, dy, dx, kind: int) -> None:
    _f32c(x, dy, dx)
    _call(lib().la_act_bwd, x, dy, dx, x.numel(), kind)


def attn_small_lse(q, k, b: int, nq: int, nk: int, heads: int, hd: int, lse) -> None:
    _call(lib().la_attn_small_lse, q, q.stride(0), k, k.stride(0), b, nq, nk, heads, hd, lse)


def attn_small_bwd(q, k, v, o, dout, lse, b: int, nq: int, nk: int, heads: int, hd: int, dq, dk, dv) -> None:
    _call(lib().la_attn_small_bwd, q, q.stride(0), k, k.stride(0), v, v.stride(0), o, dout, dout.stride(0), lse, b, nq, nk, heads, hd, dq, dk, dv)


def bilinear_rows(x, n: int, h: int, w: int, c: int, oh: int, ow: int, out) -> None:
    """la_bilinear_rows: NHWC rows [n, h * w, c] -> [n, oh * ow, c] (bilinear, align_corners=False)."""
    _f32c(x, out)
    if c % 4 or x.numel() != n * h * w * c or out.numel() != n * oh * ow * c:
        raise ValueError(f"la_bilinear_rows: [{n}, {h}x{w}, {c}] -> [{n}, {oh}x{ow}, {c}] needs c % 4 == 0 and tensors of exactly those "
                         f"sizes (got {x.numel()} and {out.numel()} elements)")
    _call(lib().la_bilinear_rows, x, n, h, w, c, out, oh, ow)


def bilinear_rows_bwd_set(dy, n: int, oh: int, ow: int, c: int, dx, ih: int, iw: int) -> None:
    """la_bilinear_rows_bwd_set: adjoint of bilinear_rows for reductions (bilinear_bwd_set_ok), dx written."""
    _f32c(dy, dx)
    if c % 4 or dy.numel() != n * oh * ow * c or dx.numel() != n * ih * iw * c or not bilinear_bwd_set_ok(oh, ow, ih, iw):
        raise ValueError(f"la_bilinear_rows_bwd_set: dy [{n}, {oh}x{ow}, {c}] -> dx [{n}, {ih}x{iw}, {c}] needs c % 4 == 0, a reduction "
                         f"the gathered adjoint takes (bilinear_bwd_set_ok) and tensors of exactly those sizes (got {dy.numel()} and {dx.numel()})")
    _call(lib().la_bilinear_rows_bwd_set, dy, n, oh, ow, c, dx, ih, iw)


def bilinear_bwd_set_ok(oh: int, ow: int, ih: int, iw: int) -> bool:
    """True when la_bilinear_bwd_set takes the shape (a reduction that fits its LDS tables): dx is then WRITTEN, not accumulated."""
    return bool(lib().la_bilinear_bwd_set_ok(oh, ow, ih, iw))


def bilinear_bwd_set(dy, n: int, oh: int, ow: int, dy_plane: int, dy_ld: int, dx, ih: int, iw: int, dx_plane: int, dx_ld: int) -> None:
    """la_bilinear_bwd_set: the adjoint of a bilinear REDUCTION as a gather (no atomics, dx written)."""
    _f32c(dy, dx)
    if n <= 0 or dy_ld < ow or dx_ld < iw or (n - 1) * dy_plane + (oh - 1) * dy_ld + ow > dy.numel() or \
            (n - 1) * dx_plane + (ih - 1) * dx_ld + iw > dx.numel() or not bilinear_bwd_set_ok(oh, ow, ih, iw):
        raise ValueError(f"la_bilinear_bwd_set: {n} planes {oh}x{ow} (plane {dy_plane}, ld {dy_ld}) -> {ih}x{iw} (plane {dx_plane}, ld {dx_ld}) "
                         f"reaches beyond the tensors ({dy.numel()} / {dx.numel()} elements) or is not a reduction the gathered adjoint takes")
    _call(lib().la_bilinear_bwd_set, dy, n, oh, ow, dy_plane, dy_ld, dx, ih, iw, dx_plane, dx_ld)


def bilinear_bwd(dy, n: int, oh: int, ow: int, dy_plane: int, dy_ld: int, dx, ih: int, iw: int, dx_plane: int, dx_ld: int) -> None:
    _call(lib().la_bilinear_bwd, dy, n, oh, ow, dy_plane, dy_ld, dx, ih, iw, dx_plane, dx_ld)


def classify_bwd(dseg, feat, protos, b: int, npix: int, c: int, cf: int, dfeat, dprotos) -> None:
    _f32c(dseg, feat, protos, dfeat, dprotos)
    _call(lib().la_classify_bwd, dseg, feat, protos, b, npix, c, cf, dfeat, dprotos)


def region_mean_bwd(dy, b: int, m: int, c: int, g: int, k: int, d: int, dx) -> None:
    """dy fp32 [b, m*k*k, c, d] -> dx fp32 [b*m*c, g*g, d] (written): every pixel gathers dy / |bin| of the bins that contain it."""
    _f32c(dy, dx)
    if dx.numel() != b * m * c * g * g * d or dy.numel() != b * m * k * k * c * d:
        raise ValueError(f"region_mean_bwd: dy must hold [{b}, {m * k * k}, {c}, {d}] and dx [{b * m * c}, {g * g}, {d}] elements "
                         f"(got {dy.numel()} and {dx.numel()})")
    _call(lib().la_region_mean_bwd, dy, b, m, c, g, k, d, dx)


def classify_max_bwd(dseg, feat, protos, win, b: int, npix: int, n: int, c: int, cf: int, dfeat, dprotos) -> None:
    """dfeat [b*npix, cf] is written, dprotos [b, n, c, cf] ACCUMULATED; win: the int32 winners classify_max returned."""
    _classify_max_args(feat, protos, b, npix, n, c, cf, ((dseg, torch.float32), (win, torch.int32)))
    _f32c(dfeat, dprotos)
    if dfeat.numel() != feat.numel() or dprotos.numel() != protos.numel():
        raise ValueError("classify_max_bwd: dfeat / dprotos must have the sizes of feat / protos")
    _call(lib().la_classify_max_bwd, dseg, feat, protos, win, b, npix, n, c, cf, dfeat, dprotos)


def row_broadcast(src, groups: int, rep: int, d: int, scale: float, out) -> None:
    _f32c(src, out)
    _call(lib().la_row_broadcast, src, groups, rep, d, scale, out)


# ---- fused image-side kernels of the two-way transformer (csrc/twoway.hip) -----------------------------------------------------
def twoway_part_size(groups: int, hw: int, nt: int, d: int) -> int:
    """fp32 elements of la_twoway_t2i's partials buffer: [groups][64-row tiles][2 row tiles of 32][nt][8 heads][2 + head width]."""
    return groups * ((hw + 63) // 64) * 2 * nt * 8 * (2 + d // 16)


def twoway_pe_layout(table: torch.Tensor) -> torch.Tensor:
    """pe @ W.T + b as fp32 [hw, D / 2] -> the same table in the order the fused two-way kernels read it (one pass, once per layer and grid)."""
    _f32c(table)
    hw, di = table.shape
    out = torch.empty(((hw + 63) // 64) * 64 * di, device=table.device)
    _call(lib().la_twoway_pe_layout, table, hw, di, out)
    return out


def twoway_t2i(img, wk, wv, pek, bv, q, groups: int, hw: int, nt: int, heads: int, part, out) -> None:
    """wk / wv: (hi, lo) fp16 plane pairs [D / 2, D]; pek = twoway_pe_layout(pe @ Wk.T + bk).  D = 256 or 512, 8 heads."""
    _f32c(img, pek, bv, q, part, out)
    d = img.shape[1]
    need = twoway_part_size(groups, hw, nt, d)
    if part.numel() < need:
        raise ValueError(f"twoway_t2i: scratch too small ({part.numel()} < {need})")
    _call(lib().la_twoway_t2i, img, wk[0], wk[1], wv[0], wv[1], pek, bv, q, groups, hw, nt, d, heads, part, out)


def twoway_i2t(img, wq, peq, k, v, wo, bo, gamma, beta, eps: float, groups: int, hw: int, nt: int, heads: int) -> None:
    """peq = twoway_pe_layout(pe @ Wq.T + bq); img is updated in place."""
    _f32c(img, peq, k, v, bo, gamma, beta)
    _call(lib().la_twoway_i2t, img, wq[0], wq[1], peq, k, v, wo[0], wo[1], bo, gamma, beta, eps, groups, hw, nt, img.shape[1], heads)


def stream_mlp_ok(d: int, h: int) -> bool:
    return bool(lib().la_stream_mlp_ok(d, h))


def stream_mlp(x, w1, b1, w2, b2, gamma, beta, eps: float, rows: Optional[int] = None, d: Optional[int] = None,
               h: Optional[int] = None) -> None:
    """x <- LN(x + relu(x W1^T + b1) W2^T + b2) in place on the fp32 stream x [rows, D].  w1 / w2: (hi, lo) fp16 plane pairs [H, D] /
    [D, H].  rows / d / h default to the tensors' shapes (the refusal tests pass them)."""
    _f32c(x, b1, b2, gamma, beta)
    rows = (x.shape[0] if x is not None else 0) if rows is None else rows
    d = x.shape[1] if d is None else d
    h = b1.shape[0] if h is None else h
    _call(lib().la_stream_mlp, x, w1[0], w1[1], b1, w2[0], w2[1], b2, gamma, beta, eps, rows, d, h)


# ---- image-encoder backward ---------------------------------------------------------------------------
def attn_fwd_lse(qkv, vt, out16, lse, b: int, heads: int, t: int, tpad: int, e: int, scale: float) -> None:
    _call(lib().la_attn_fwd_lse, qkv, vt, out16, lse, b, heads, t, tpad, e, scale, dt_of(qkv))


def head_transpose(src, col0: int, b: int, heads: int, t: int, tpad: int, dst) -> None:
    _call(lib().la_head_transpose, src, src.stride(0), col0, b, heads, t, tpad, dst, dt_of(src))


def attn_bwd(qkv, out16, dout16, kt, qt, dot, lse, dvec, dqkv, b: int, heads: int, t: int, tpad: int, e: int, scale: float) -> None:
    _call(lib().la_attn_bwd, qkv, out16, dout16, kt, qt, dot, lse, dvec, dqkv, b, heads, t, tpad, e, scale, dt_of(qkv))


def attn_fwd_relpos_lse(qkv, vt, out16, relh, relw, lse, b: int, heads: int, t: int, tpad: int, g: int, e: int, scale: float) -> None:
    _call(lib().la_attn_fwd_relpos_lse, qkv, vt, out16, relh, relw, lse, b, heads, t, tpad, g, e, scale, dt_of(qkv))


def attn_bwd_relpos(qkv, out16, dout16, kt, qt, dot, lse, dvec, dqkv, relh, relw, drelh, drelw, b: int, heads: int, t: int, tpad: int, g: int,
                    e: int, scale: float) -> None:
    _call(lib().la_attn_bwd_relpos, qkv, out16, dout16, kt, qt, dot, lse, dvec, dqkv, relh, relw, drelh, drelw, b, heads, t, tpad, g, e, scale,
          dt_of(qkv))


def relpos_bwd(qkv, dqkv, drelh, drelw, tabh, tabw, dtabh, dtabw, b: int, heads: int, g: int, e: int, gscale: float = 1.0) -> None:
    _call(lib().la_relpos_bwd, qkv, dqkv, drelh, drelw, tabh, tabw, dtabh, dtabw, b, heads, g, e, gscale, dt_of(qkv))


def cast(src, dst, scale: float = 1.0) -> None:
    """dst = scale * src (fp32 <-> 16-bit, or fp32 -> fp32 possibly in place); contiguous tensors of equal numel."""
    if not (src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()):
        raise ValueError("la_cast needs contiguous tensors of equal size")
    _call(lib().la_cast, src, dt_of(src), dst, dt_of(dst), src.numel(), scale)


def gelu_fwd16(pre16, post16) -> None:
    """post16 = GELU(pre16), contiguous 16-bit tensors of equal size (numel % 8 == 0)."""
    if not (pre16.is_contiguous() and post16.is_contiguous() and pre16.numel() == post16.numel() and pre16.dtype == post16.dtype):
        raise ValueError("gelu_fwd16 needs contiguous 16-bit tensors of equal size and dtype")
    _call(lib().la_gelu_fwd16, pre16, post16, pre16.numel(), dt_of(pre16))


def gelu_bwd16(pre16, dh, d32=None, d16=None) -> None:
    _call(lib().la_gelu_bwd16, pre16, dh, d32, d16, pre16.numel(), dt_of(pre16))


def axpy(x, y, a: float) -> None:
    """y += a * x (contiguous fp32)."""
    _f32c(x, y)
    _call(lib().la_axpy, x, y, x.numel(), a)


def transpose16(src, dst, colsum=None) -> None:
    """dst[c, r] = src[r, c]; src fp32 / 16-bit [R, C] (row stride src.stride(0)), dst 16-bit [C, Rp] with Rp >= R, Rp % 64 == 0 (zero padded).
    colsum: optional fp32 [C] that receives += the column sums of the (16-bit) values written - the bias gradient of the layer whose
    output gradient is being transposed."""
    r, c = src.shape
    if src.stride(1) != 1 or not dst.is_contiguous() or dst.shape[0] != c:
        raise ValueError("transpose16: src needs unit column stride, dst contiguous [C, Rp]")
    if colsum is not None and (colsum.dtype != torch.float32 or colsum.numel() != c or not colsum.is_contiguous()):
        raise ValueError("transpose16: colsum must be contiguous fp32 [C]")
    _call(lib().la_transpose16, src, dt_of(src), src.stride(0), r, c, dst, dt_of(dst), dst.shape[1], colsum)


# ---- fp8 QK^T attention (opt-in) --------------------------------------------------------------------------
def qk_fp8(qkv, e: int, qk8) -> None:
    _call(lib().la_qk_fp8, qkv, qkv.shape[0], e, qk8, dt_of(qkv))


def add_rowvec_split(x, v, rows_per_group: int, split16) -> None:
    """x[r] += v[r / rows_per_group] in place (v may be None) and split16 [rows, 2 D] fp16 = [hi | lo] planes of the result."""
    _f32c(x, v)
    if split16.dtype != torch.float16 or tuple(split16.shape) != (x.shape[0], 2 * x.shape[1]) or not split16.is_contiguous():
        raise ValueError("add_rowvec_split: split16 must be a contiguous fp16 [rows, 2 D] buffer")
    _call(lib().la_add_rowvec_split, x, v, x.shape[0], rows_per_group, x.shape[1], split16)


def attn_fwd_fp8(qk8, vt, out16, b: int, heads: int, t: int, tpad: int, e: int, scale: float) -> None:
    _call(lib().la_attn_fwd_fp8, qk8, vt, out16, b, heads, t, tpad, e, scale, dt_of(out16))


# ---- token-mean correction of single-plane weights ---------------------------------------------------------
def colmean16(src, groups: int, rows_per_group: int, out, scratch, wpart: int = 0, h: int = 0, w: int = 0) -> None:
    """out[g] = mean of the rows of group g (fp32 [groups, D]); scratch fp32 >= groups * ceil(rows_per_group / 128) * D elements;
    wpart: src window-partitioned, rows gathered in image order."""
    need = groups * ((rows_per_group + 127) // 128) * src.shape[1]
    if scratch.numel() < need or scratch.dtype != torch.float32:
        raise ValueError(f"colmean16 scratch needs {need} fp32 elements")
    _call(lib().la_colmean16, src, src.stride(0), groups, rows_per_group, src.shape[1], out, scratch, wpart, h, w, dt_of(src))


LN_CS_ROWS = 32        # rows per column-sum partial of la_layernorm_g (norm.hip)


def ln_cs_chunks(rows_per_group: int) -> int:
    return (rows_per_group + LN_CS_ROWS - 1) // LN_CS_ROWS


def layernorm_g(x, xg, rows_per_group: int, gamma, beta, eps: float, *, out32=None, out16=None, window=0, H=0, W=0, colsum_part=None,
                dt=LA_F16) -> None:
    """colsum_part: fp32, >= (rows / rows_per_group) * ln_cs_chunks(rows_per_group) * E elements (column sums of the stored rows per
    fixed share of a group; colsum_fold makes the means)."""
    rows, e = x.shape
    if colsum_part is not None:
        need = rows // rows_per_group * ln_cs_chunks(rows_per_group) * e
        if colsum_part.dtype != torch.float32 or colsum_part.numel() < need:
            raise ValueError(f"layernorm_g colsum_part needs {need} fp32 elements")
    _call(lib().la_layernorm_g, x, xg, rows_per_group, x.stride(0), rows, e, gamma, beta, eps, out32, out16, window, H, W, colsum_part, dt)


def attn_fwd_cs(qkv, vt, out16, relh, relw, b: int, heads: int, t: int, tpad: int, g: int, e: int, scale: float, mode: int, cspart,
                cs_h: int = 0, cs_w: int = 0, tabh=None, tabw=None) -> None:
    """attn_fwd + column sums of every 128-query block of the output: cspart fp32 [b * ceil(t / 128), e]."""
    need = b * ((t + 127) // 128) * e
    if cspart.dtype != torch.float32 or cspart.numel() < need:
        raise ValueError(f"attn_fwd_cs cspart needs {need} fp32 elements")
    _call(lib().la_attn_fwd_cs, qkv, vt, out16, relh, relw, tabh, tabw, b, heads, t, tpad, g, e, scale, mode, cspart, cs_h, cs_w, dt_of(qkv))


def attn_fwd_rows(qkv, out16, b: int, heads: int, t: int, tpad: int, g: int, e: int, scale: float, mode: int, tabh=None, tabw=None,
                  cspart=None, img_hw=None, padrow=None) -> None:
    """Attention without a V^T copy (la_attn_fwd_rows): V tiles row-major from the v columns of qkv.  img_hw = (H, W) + padrow: SAM windows
    addressed in image order (b = images * windows per image)."""
    if qkv.dtype not in (torch.float16, torch.bfloat16) or out16.dtype != qkv.dtype or not (qkv.is_contiguous() and out16.is_contiguous()):
        raise ValueError("attn_fwd_rows: qkv / out16 must be contiguous 16-bit tensors of one dtype")
    if cspart is not None:
        need = b * ((t + 127) // 128) * e
        if cspart.dtype != torch.float32 or cspart.numel() < need:
            raise ValueError(f"attn_fwd_rows cspart needs {need} fp32 elements")
    ih, iw = (0, 0) if img_hw is None else img_hw
    if padrow is not None and (padrow.dtype != qkv.dtype or padrow.numel() != 3 * e or not padrow.is_contiguous()):
        raise ValueError("attn_fwd_rows: padrow must be a contiguous [3E] row of the qkv dtype")
    _call(lib().la_attn_fwd_rows, qkv, out16, tabh, tabw, b, heads, t, tpad, g, e, scale, mode, cspart, ih, iw, padrow, dt_of(qkv))


def colsum_fold(part, groups: int, chunks: int, d: int, inv: float, out) -> None:
    """out[g, :d] = inv * sum_j part[g * chunks + j, :d] (out: fp32 rows of stride out.stride(0), e.g. a column slice)."""
    if out.dtype != torch.float32 or out.stride(1) != 1 or out.shape[0] < groups or out.shape[1] < d:
        raise ValueError("colsum_fold: out must be fp32 [groups, >= d] with unit column stride")
    _call(lib().la_colsum_fold, part, groups, chunks, d, inv, out, out.stride(0))


def add_rowvec(x, v, rows_per_group: int) -> None:
    _f32c(x, v)
    _call(lib().la_add_rowvec, x, v, x.shape[0], rows_per_group, x.shape[1])


# ---- the two-level classification head (classification_levels = 2, csrc/levels.hip) ----------------------------------------------------
def _numel(what: str, **named) -> None:
    for name, (t, n) in named.items():
        if t.numel() != n:
            raise ValueError(f"{what}: {name} must hold {n} elements (got {t.numel()})")


def classify_wide(tok, img, b: int, npix: int, c: int, d: int, seg) -> None:
    """seg[b, c, pix] = tok[b, c, :] . img[b, pix, :] over the transformer width d (d % 64 == 0, d <= 1024, c <= 32: the library refuses
    anything else)."""
    _f32c(tok, img, seg)
    _numel("classify_wide", tok=(tok, b * c * d), img=(img, b * npix * d), seg=(seg, b * c * npix))
    _call(lib().la_classify_wide, tok, img, b, npix, c, d, seg)


def classify_wide_bwd(dseg, tok, img, b: int, npix: int, c: int, d: int, dimg, dtok) -> None:
    """dimg [b, npix, d] is written, dtok [b, c, d] ACCUMULATED."""
    _f32c(dseg, tok, img, dimg, dtok)
    _numel("classify_wide_bwd", dseg=(dseg, b * c * npix), tok=(tok, b * c * d), img=(img, b * npix * d), dimg=(dimg, b * npix * d),
           dtok=(dtok, b * c * d))
    _call(lib().la_classify_wide_bwd, dseg, tok, img, b, npix, c, d, dimg, dtok)


def level_reduce(cls0, cls1, w, bias, b: int, c: int, gh: int, gw: int, seg) -> None:
    """seg [b, c, 4gh, 4gw] = bias + conv3x3 (zero padding) of [cls0, x4 bilinear enlargement of cls1 [b, c, gh, gw]] with w [2][3][3]."""
    _f32c(cls0, cls1, w, bias, seg)
    _numel("level_reduce", cls0=(cls0, b * c * 16 * gh * gw), cls1=(cls1, b * c * gh * gw), w=(w, 18), bias=(bias, 1),
           seg=(seg, b * c * 16 * gh * gw))
    _call(lib().la_level_reduce, cls0, cls1, w, bias, b, c, gh, gw, seg)


def level_reduce_bwd(dseg, cls0, cls1, w, b: int, c: int, gh: int, gw: int, dcls0, dcls1, dw, dbias) -> None:
    """dcls0 [b, c, 4gh, 4gw] and dcls1 [b, c, gh, gw] are written; dw [18] and dbias [1] ACCUMULATED."""
    _f32c(dseg, cls0, cls1, w, dcls0, dcls1, dw, dbias)
    n0, n1 = b * c * 16 * gh * gw, b * c * gh * gw
    _numel("level_reduce_bwd", dseg=(dseg, n0), cls0=(cls0, n0), cls1=(cls1, n1), w=(w, 18), dcls0=(dcls0, n0), dcls1=(dcls1, n1),
           dw=(dw, 18), dbias=(dbias, 1))
    _call(lib().la_level_reduce_bwd, dseg, cls0, cls1, w, b, c, gh, gw, dcls0, dcls1, dw, dbias)


# ---- conv_classification (prototype_tconv + the 5 x 5 per-episode correlation, csrc/convcls.hip) ----------------------------------------
def proto_kernels(protos, w1, w2, bc: int, cf: int, k1, k) -> None:
    """protos [bc, cf] through the two ConvTranspose2d(cf, cf, 3) weights w1, w2 (in, out, ky, kx): k1 [bc, cf, 3, 3] (kept for the
    backward) and k [bc, 25, cf], tap-major and channel-minor.  cf a multiple of 32 up to 256: the library refuses anything else."""
    _f32c(protos, w1, w2, k1, k)
    _numel("proto_kernels", protos=(protos, bc * cf), w1=(w1, 9 * cf * cf), w2=(w2, 9 * cf * cf), k1=(k1, bc * cf * 9), k=(k, bc * 25 * cf))
    _call(lib().la_proto_kernels, protos, w1, w2, bc, cf, k1, k)


def proto_kernels_bwd(dk, protos, k1, w1, w2, bc: int, cf: int, dk1, dprotos, dw1, dw2) -> None:
    """dk1 [bc, cf, 3, 3] (scratch) and dprotos [bc, cf] are written; dw1, dw2 ACCUMULATED."""
    _f32c(dk, protos, k1, w1, w2, dk1, dprotos, dw1, dw2)
    _numel("proto_kernels_bwd", dk=(dk, bc * 25 * cf), protos=(protos, bc * cf), k1=(k1, bc * cf * 9), w1=(w1, 9 * cf * cf),
           w2=(w2, 9 * cf * cf), dk1=(dk1, bc * cf * 9), dprotos=(dprotos, bc * cf), dw1=(dw1, 9 * cf * cf), dw2=(dw2, 9 * cf * cf))
    _call(lib().la_proto_kernels_bwd, dk, protos, k1, w1, w2, bc, cf, dk1, dprotos, dw1, dw2)


def classify_conv(feat, k, b: int, c: int, h: int, w: int, cf: int, seg) -> None:
    """seg [b, c, h, w] = the 5 x 5 cross-correlation (zero padding 2) of feat NHWC [b, h, w, cf] with episode b's kernels k [b, c, 25, cf]."""
    _f32c(feat, k, seg)
    _numel("classify_conv", feat=(feat, b * h * w * cf), k=(k, b * c * 25 * cf), seg=(seg, b * c * h * w))
    _call(lib().la_classify_conv, feat, k, b, c, h, w, cf, seg)


def classify_conv_bwd(dseg, feat, k, b: int, c: int, h: int, w: int, cf: int, dfeat, dk) -> None:
    """dfeat [b, h, w, cf] and dk [b, c, 25, cf] are both written; the same input gives the same bits."""
    _f32c(dseg, feat, k, dfeat, dk)
    _numel("classify_conv_bwd", dseg=(dseg, b * c * h * w), feat=(feat, b * h * w * cf), k=(k, b * c * 25 * cf),
           dfeat=(dfeat, b * h * w * cf), dk=(dk, b * c * 25 * cf))
    _call(lib().la_classify_conv_bwd, dseg, feat, k, b, c, h, w, cf, dfeat, dk)


# ---- embedding_extraction = "cross_attention" (the folded attention over the stream, csrc/extract.hip) ---------------------------------
EXTRACT_HEADS = 8


def extract_pool_plan(m: int, hw: int, d: int, r: int):
    """(split_rows, nsplit, scratch floats per pair) of ``extract_pool`` for m slabs of hw rows, width d and r = 8 n folded queries: the
    rows of a pair are cut into nsplit pieces of split_rows rows.  A function of these four sizes only."""
    split, ns, per = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _call(lib().la_extract_pool_plan, m, hw, d, r, C.byref(split), C.byref(ns), C.byref(per))
    return split.value, ns.value, per.value


def extract_pool(x, qt, b: int, m: int, c: int, hw: int, d: int, n: int, scratch, out) -> None:
    """out [b c, 8 n, d] = softmax-weighted means of the m hw stream rows of every pair under the folded queries qt ([b c, 8 n, d], or
    one [8 n, d] block for all pairs).  scratch: fp32, at least b c times the per-pair size of ``extract_pool_plan``."""
    _f32c(x, qt, scratch, out)
    bcast = _extract_pool_sizes("extract_pool", x, qt, out, scratch, extract_pool_plan, b, m, c, hw, d, n)
    _call(lib().la_extract_pool, x, qt, 1 if bcast else 0, b, m, c, hw, d, n, scratch, out)


def extract_fold(q, wk, bc: int, n: int, d: int, qt) -> None:
    """qt [bc, 8 n, d], row h n + j = W_k,h^T q[z n + j, head h] / sqrt(d / 16)."""
    _f32c(q, wk, qt)
    _numel("extract_fold", q=(q, bc * n * (d // 2)), wk=(wk, (d // 2) * d), qt=(qt, bc * EXTRACT_HEADS * n * d))
    _call(lib().la_extract_fold, q, wk, bc, n, d, qt)


def extract_unfold(pooled, wv, bv, bc: int, n: int, d: int, o) -> None:
    """o [bc n, d / 2]: column h hd + e of row z n + j = W_v[h hd + e] . pooled[z, h n + j] + b_v[h hd + e]."""
    _f32c(pooled, wv, bv, o)
    _numel("extract_unfold", pooled=(pooled, bc * EXTRACT_HEADS * n * d), wv=(wv, (d // 2) * d), bv=(bv, d // 2), o=(o, bc * n * (d // 2)))
    _call(lib().la_extract_unfold, pooled, wv, bv, bc, n, d, o)


# ---- training of the extraction (csrc/extract_bwd.hip) --------------------------------------------------------------------------------
def _extract_pool_sizes(who: str, x, qt, out, scratch, plan, b: int, m: int, c: int, hw: int, d: int, n: int) -> bool:
    """The size checks of the three passes over the stream (``plan``: the pass's own scratch plan) -> qt is the broadcast form."""
    r = EXTRACT_HEADS * n
    if x.numel() != b * m * c * hw * d or out.numel() != b * c * r * d or qt.numel() not in (r * d, b * c * r * d):
        raise ValueError(f"{who}: x must hold [{b * m * c}, {hw}, {d}], qt [{b * c}, {r}, {d}] or [{r}, {d}] and out [{b * c}, {r}, {d}] "
                         f"elements (got {x.numel()}, {qt.numel()}, {out.numel()})")
    if 1 <= n <= 16 and d in (64, 128, 256):
        need = b * c * plan(m, hw, d, r)[2]
        if scratch.numel() < need:
            raise ValueError(f"{who}: scratch holds {scratch.numel()} floats, {need} needed")
    return qt.numel() == r * d and b * c != 1


def extract_pool_lse(x, qt, b: int, m: int, c: int, hw: int, d: int, n: int, scratch, out, lse) -> None:
    """``extract_pool`` (the same kernels, ``out`` bit-identical) which also writes lse [b c, 8 n] = max + log(sum) of every folded query's
    scores: what ``extract_pool_bwd`` rebuilds the softmax weights from."""
    _f32c(x, qt, scratch, out, lse)
    bcast = _extract_pool_sizes("extract_pool_lse", x, qt, out, scratch, extract_pool_plan, b, m, c, hw, d, n)
    _numel("extract_pool_lse", lse=(lse, b * c * EXTRACT_HEADS * n))
    _call(lib().la_extract_pool_lse, x, qt, 1 if bcast else 0, b, m, c, hw, d, n, scratch, out, lse)


def extract_pool_bwd_plan(m: int, hw: int, d: int, r: int):
    """(tile_rows, ntiles, scratch floats per pair) of ``extract_pool_bwd``: one workgroup per tile of tile_rows stream rows of a pair.  A
    function of these four sizes only."""
    rows, nt, per = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _call(lib().la_extract_pool_bwd_plan, m, hw, d, r, C.byref(rows), C.byref(nt), C.byref(per))
    return rows.value, nt.value, per.value


def extract_pool_bwd(x, qt, out, lse, dout, b: int, m: int, c: int, hw: int, d: int, n: int, scratch, dx, dqt) -> None:
    """dx (the layout of x) and dqt (the layout of qt: [b c, 8 n, d], or [8 n, d] summed over the pairs in the broadcast form) from
    dout [b c, 8 n, d]; out and lse as ``extract_pool_lse`` left them.  Both are written.  scratch: fp32, at least b c times the
    per-pair size of ``extract_pool_bwd_plan``."""
    _f32c(x, qt, out, lse, dout, scratch, dx, dqt)
    r = EXTRACT_HEADS * n
    _numel("extract_pool_bwd", lse=(lse, b * c * r), dout=(dout, b * c * r * d), dx=(dx, x.numel()), dqt=(dqt, qt.numel()))
    bcast = _extract_pool_sizes("extract_pool_bwd", x, qt, out, scratch, extract_pool_bwd_plan, b, m, c, hw, d, n)
    _call(lib().la_extract_pool_bwd, x, qt, 1 if bcast else 0, out, lse, dout, b, m, c, hw, d, n, scratch, dx, dqt)


def extract_fold_bwd(dqt, q, wk, bc: int, n: int, d: int, dq, dwk, dbk) -> None:
    """dq [bc n, d / 2] is written (with the 1 / sqrt(d / 16) factor), dwk [d / 2, d] is ADDED to, dbk [d / 2] is written as zero (the key
    bias cancels in the softmax)."""
    _f32c(dqt, q, wk, dq, dwk, dbk)
    _numel("extract_fold_bwd", dqt=(dqt, bc * EXTRACT_HEADS * n * d), q=(q, bc * n * (d // 2)), wk=(wk, (d // 2) * d), dq=(dq, bc * n * (d // 2)),
           dwk=(dwk, (d // 2) * d), dbk=(dbk, d // 2))
    _call(lib().la_extract_fold_bwd, dqt, q, wk, bc, n, d, dq, dwk, dbk)


def extract_unfold_bwd(do, pooled, wv, bc: int, n: int, d: int, dpooled, dwv, dbv) -> None:
    """dpooled [bc, 8 n, d] is written; dwv [d / 2, d] and dbv [d / 2] are ADDED to."""
    _f32c(do, pooled, wv, dpooled, dwv, dbv)
    _numel("extract_unfold_bwd", do=(do, bc * n * (d // 2)), pooled=(pooled, bc * EXTRACT_HEADS * n * d), wv=(wv, (d // 2) * d),
           dpooled=(dpooled, bc * EXTRACT_HEADS * n * d), dwv=(dwv, (d // 2) * d), dbv=(dbv, d // 2))
    _call(lib().la_extract_unfold_bwd, do, pooled, wv, bc, n, d, dpooled, dwv, dbv)


# ---- rotary position embedding (DINOv3 ViT) -----------------------------------------------------------------
def rope_qk(qkv, tokens: int, prefix: int, heads: int, hd: int, hdp: int, cos, sin) -> None:
    """Rotate, in place, the q and k columns of the packed 16-bit q | k | v buffer qkv [rows, >= 3 heads hdp] (row stride = ld): the rows
    of every image of ``tokens`` rows from ``prefix`` on, the first hd of the hdp columns of every head, by the fp32 tables cos, sin
    [tokens - prefix, hd].  Everything else keeps its bits."""
    _f32c(cos, sin)
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("rope_qk: qkv must be a 16-bit [rows, ld] matrix with unit column stride")
    if tuple(cos.shape) != (tokens - prefix, hd) or tuple(sin.shape) != (tokens - prefix, hd):
        raise ValueError(f"rope_qk: cos and sin must be [tokens - prefix, hd] = [{tokens - prefix}, {hd}]")
    if qkv.shape[1] < 3 * heads * hdp:
        raise ValueError(f"rope_qk: qkv has {qkv.shape[1]} columns, q | k | v of {heads} heads of {hdp} need {3 * heads * hdp}")
    _call(lib().la_rope_qk, qkv, qkv.shape[0], qkv.stride(0), tokens, prefix, heads, hd, hdp, cos, sin, dt_of(qkv))


# ---- cosine-similarity few-shot segmenter (csrc/similarity.hip) ----------------------------------------------
SIM_MAX_CLASSES = 32        # one class word per support pixel


def _sim_width(who: str, d: int) -> None:
    if d % 64 or not 64 <= d <= 1024:
        raise ValueError(f"{who}: feature width D = {d} must be a multiple of 64 in [64, 1024]")


def _sim_classes(who: str, n: int) -> None:
    if not 1 <= n <= SIM_MAX_CLASSES:
        raise ValueError(f"{who}: N = {n} classes, a class word holds 1 .. {SIM_MAX_CLASSES}")


def sim_prepare(x, gin: int, cs: int, out16) -> None:
    """x fp32 NHWC rows [n, gin^2, D] -> out16 fp16 [n, cs^2, D]: the bicubic resample to cs x cs (none if gin == cs), the L2
    normalisation over D and the rounding, in one pass."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[1] != gin * gin:
        raise ValueError(f"sim_prepare: x must be a contiguous fp32 [n, gin^2 = {gin * gin}, D] tensor, got {x.dtype} {tuple(x.shape)}")
    n, _, d = x.shape
    _sim_width("sim_prepare", d)
    if out16.dtype != torch.float16 or not out16.is_contiguous() or tuple(out16.shape) != (n, cs * cs, d):
        raise ValueError(f"sim_prepare: out16 must be a contiguous fp16 [{n}, {cs * cs}, {d}] tensor, got {out16.dtype} {tuple(out16.shape)}")
    _call(lib().la_sim_prepare, x, n, gin, cs, d, out16)


def sim_class_bits(masks, cs: int, bits) -> None:
    """masks fp32 [P, N, Hm, Wm] -> bits int32 [P, cs^2] (the bit pattern of a uint32 class word): bit n = the nearest source pixel of
    class n is non-zero, bit 0 = none of the classes 1 .. N - 1 has the pixel."""
    if masks.dim() != 4 or masks.dtype != torch.float32 or not masks.is_contiguous():
        raise ValueError("sim_class_bits: masks must be a contiguous fp32 [P, N, Hm, Wm] tensor")
    p, n, hm, wm = masks.shape
    _sim_classes("sim_class_bits", n)
    if bits.dtype != torch.int32 or not bits.is_contiguous() or tuple(bits.shape) != (p, cs * cs):
        raise ValueError(f"sim_class_bits: bits must be a contiguous int32 [{p}, {cs * cs}] tensor, got {bits.dtype} {tuple(bits.shape)}")
    _call(lib().la_sim_class_bits, masks, p, n, hm, wm, cs, bits)


def sim_max_plan(b: int, q: int, k: int, d: int, n: int, ncu: int = 0):
    """(key split, floats of workspace) of ``sim_max`` on a device of ncu compute units (<= 0: the current device)."""
    _sim_width("sim_max_plan", d)
    _sim_classes("sim_max_plan", n)
    ks, wf = C.c_int(0), C.c_longlong(0)
    _call(lib().la_sim_max_plan, b, q, k, d, n, ncu, C.byref(ks), C.byref(wf))
    return ks.value, wf.value


def sim_max(q16, k16, bits, n: int, out, work=None) -> None:
    """out[b, c, q] = max over the keys k whose class word bits[b, k] has bit c of <q16[b, q], k16[b, k]> (-inf: no such key).
    q16 fp16 [B, Q, D], k16 fp16 [B, K, D], bits int32 [B, K], out fp32 [B, n, Q]; work: fp32, at least ``sim_max_plan(...)[1]`` floats
    (allocated here if not given)."""
    for t, name in ((q16, "q16"), (k16, "k16")):
        if t.dim() != 3 or t.dtype != torch.float16 or not t.is_contiguous():
            raise ValueError(f"sim_max: {name} must be a contiguous fp16 [B, rows, D] tensor, got {t.dtype} {tuple(t.shape)}")
    b, q, d = q16.shape
    k = k16.shape[1]
    _sim_width("sim_max", d)
    _sim_classes("sim_max", n)
    if k16.shape[0] != b or k16.shape[2] != d:
        raise ValueError(f"sim_max: k16 {tuple(k16.shape)} does not go with q16 {tuple(q16.shape)}")
    if bits.dtype != torch.int32 or not bits.is_contiguous() or tuple(bits.shape) != (b, k):
        raise ValueError(f"sim_max: bits must be a contiguous int32 [B, K] = [{b}, {k}] tensor, got {bits.dtype} {tuple(bits.shape)}")
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (b, n, q):
        raise ValueError(f"sim_max: out must be a contiguous fp32 [{b}, {n}, {q}] tensor, got {out.dtype} {tuple(out.shape)}")
    for t in (q16, k16, bits, out):
        _dev(t)
    need = sim_max_plan(b, q, k, d, n)[1]
    if work is None:
        work = torch.empty(max(need, 1), device=out.device, dtype=torch.float32)
    elif work.dtype != torch.float32 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"sim_max: work must be contiguous fp32 with at least {need} elements")
    _call(lib().la_sim_max, q16, k16, bits, b, q, k, d, n, work, work.numel(), out)
