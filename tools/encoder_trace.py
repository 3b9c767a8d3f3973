#!/usr/bin/env python
"""Launch trace of the image-encoder drivers, on the CPU.

Every public function of ``labelanything_amd._lib`` is replaced by a recorder, so ``LamEngine.encode_images`` runs without a GPU and
leaves one line per launch: the function and every argument that is not at its default, under the name the launcher's signature gives
it (a positional and a keyword spelling of one argument are the same launch); for a tensor its shape, dtype, strides, storage (numbered
by first appearance in the trace) and storage offset.  A last line holds what the encoder returned.  Two drivers with the same trace
launch the same kernels with the same arguments, in the same order, on the same buffers and aliases - what
tests/test_encoder_trace_cpu.py pins for the matrix below.

A second matrix (``train_matrix``) does the same for the TRAINING graphs of ``train_encoder.py``: forward, then backward of an all-ones
gradient, with the gradient slots laid out in one flat buffer as FlatAdamW does.  Each of its rows is pinned twice: the full trace, and
a shape trace whose storage numbers are masked (which launches, on which shapes - whatever the buffers alias).

A third matrix (``decoder_matrix``) does it for the DECODER half of ``LamEngine``: ``prompt_encoder``, ``mask_decoder`` and
``postprocess_dev`` on zero tensors, called as ``Lam._run`` calls them, pinned twice like the training rows.  The host predicates that ask
the shared library (la_conv3x3_split_ok, la_stream_mlp_ok, la_extract_pool_plan) are stand-ins whose answers the row states; the last line
holds every tensor of the prompt encoder's result and of the output - which are views of arena buffers, which clones.

  python tools/encoder_trace.py --table             name, number of calls, sha256 of the trace for the whole matrix
  python tools/encoder_trace.py --train-table       the same for the training matrix: full and shape digest per row
  python tools/encoder_trace.py --decoder-table     the same for the decoder matrix
  python tools/encoder_trace.py --print NAME        one trace (a row of any of the three matrices)
  python tools/encoder_trace.py --packed NAME       key, shape, dtype, sha256 of the bytes of every packed weight of NAME's engine, then
                                                    of its fp32 ``image_encoder.`` weights (the LayerScale products live there)
"""
from __future__ import annotations

import argparse
import hashlib
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from labelanything_amd import _lib as L                                            # noqa: E402
from labelanything_amd.config import EncoderSpec, LamConfig, encoder_kind, register_encoder     # noqa: E402

# host arithmetic only: these keep working.  (The host predicates that ask the shared library - gemm_fused_act_ok, conv3x3_split_ok,
# stream_mlp_ok, extract_pool_plan - are recorder stand-ins like the launchers: a row states their answers in ``returns``.)
PURE = ("ln_cs_chunks", "norm_cs_chunks", "twoway_part_size", "dt_of")
LAUNCHERS = {n: inspect.signature(f) for n, f in vars(L).items()
             if not n.startswith("_") and n not in PURE and inspect.isfunction(f) and f.__module__ == L.__name__}
# the ``**epilogue`` keywords of gemm / gemm_plan are those of _gemm_epilogue, defaults included
EPILOGUE = {k: v.default for k, v in inspect.signature(L._gemm_epilogue).parameters.items() if v.kind is v.KEYWORD_ONLY}


def _is_default(v, default) -> bool:
    return not isinstance(v, torch.Tensor) and type(v) is type(default) and v == default


class Recorder:
    """Stands in for the library: ``patch(setattr)`` replaces every public function of ``_lib`` with one that appends a line here."""

    def __init__(self, returns=None):
        self.lines = []
        self.shape_lines = []    # the same trace with the storage numbers masked
        self.returns = returns or {}          # launcher name -> what its stand-in returns (default None)
        self._storages = {}
        self._keep = []          # a freed storage's address would be reused and renumber the trace: hold every tensor seen

    def _fmt(self, v, mask: bool = False) -> str:
        if isinstance(v, torch.Tensor):
            self._keep.append(v)
            n = self._storages.setdefault(v.untyped_storage().data_ptr(), len(self._storages))
            return f"T({tuple(v.shape)},{str(v.dtype)[6:]},{tuple(v.stride())},s{'*' if mask else n}+{v.storage_offset()})"
        if isinstance(v, (tuple, list)):
            return "(" + ",".join(self._fmt(x, mask) for x in v) + ")"
        return repr(v)

    def note(self, head: str, items) -> None:
        """One trace line: ``head`` and (name, value) pairs, in the full and in the shape trace."""
        for lines, mask in ((self.lines, False), (self.shape_lines, True)):
            lines.append(" ".join([head] + [f"{k}={self._fmt(v, mask)}" if k else self._fmt(v, mask) for k, v in items]))

    def _stub(self, name: str):
        def call(*args, **kw):
            # arguments by the NAME the launcher gives them, so that a positional and a keyword spelling, or a default written out and
            # one left out, record the same launch: signature order, then the other keywords sorted; defaults are not printed
            named = LAUNCHERS[name].bind(*args, **kw).arguments
            extra = named.pop("epilogue", {})
            items = [(k, v) for k, v in named.items() if not _is_default(v, LAUNCHERS[name].parameters[k].default)]
            items += [(k, extra[k]) for k in sorted(extra) if not _is_default(extra[k], EPILOGUE[k])]
            self.note(name, items)
            return args[0] if name == "twoway_pe_layout" else self.returns.get(name)
        return call

    def patch(self, setattr_) -> None:
        """setattr_(module, name, value): ``monkeypatch.setattr`` in the tests (restored afterwards), plain ``setattr`` in the tool."""
        for name in LAUNCHERS:
            setattr_(L, name, (lambda: None) if name == "lib" else self._stub(name))

    def digest(self, shape: bool = False):
        lines = self.shape_lines if shape else self.lines
        return len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _wide(kind: str, depth: int, **kw) -> EncoderSpec:
    return EncoderSpec(kind, dim=768, depth=depth, heads=12, mlp=3072, **kw)


def _specs() -> None:
    import tests.cases          # noqa: F401  (registers sam_tiny, hf_tiny)
    import tests.cases_dinov2   # noqa: F401  (dinov2_tiny, dinov2_hd32, dinov2_fold)
    import tests.cases_dinov3   # noqa: F401  (dinov3_tiny, dinov3_hd32, dinov3_fold)
    for s in (1024, 448, 256):
        register_encoder(f"trace_sam_{s}", _wide("sam", 3, img_size=s, global_idx=(2,), window=14))
    register_encoder("trace_sam_640_w20", _wide("sam", 3, img_size=640, global_idx=(2,), window=20))
    register_encoder("trace_sam_hd80", EncoderSpec("sam", dim=160, depth=2, heads=2, mlp=320, img_size=448, global_idx=(1,), window=14,
                                                   out_chans=64))
    register_encoder("trace_hf", _wide("hf", 2, img_size=224))
    register_encoder("trace_hf_hd32", EncoderSpec("hf", dim=128, depth=2, heads=4, mlp=256, img_size=224))


def _sam(size: int, enc=None, ctor=None, attrs=None, last=False, **cfg):
    cfg.setdefault("image_embed_dim", 256)
    return dict(cfg=dict(encoder=enc or f"trace_sam_{size}", image_size=size, embed_dim=64, **cfg), ctor=ctor or {}, attrs=attrs or {},
                last=last)


def _hf(size: int, enc="trace_hf", attrs=None, dim=768):
    return dict(cfg=dict(encoder=enc, image_size=size, image_embed_dim=dim, embed_dim=64), ctor={}, attrs=attrs or {}, last=False)


def _vit(enc: str, size: int, attrs=None):
    """A row of an encoder whose patch size and width come from its spec (the DINO families)."""
    from labelanything_amd.config import ENCODER_SPECS
    _specs()
    spec = ENCODER_SPECS[enc]
    return dict(cfg=dict(encoder=enc, image_size=size, vit_patch_size=spec.patch, image_embed_dim=spec.dim, embed_dim=64), ctor={},
                attrs=attrs or {}, last=False)


def matrix() -> dict:
    """name -> configuration.  Two images each; see the module docstring of tests/test_encoder_trace_cpu.py for what each row reaches."""
    from labelanything_amd.engine import PRECISE_WIDE_PLANES
    nofold = {"norm_fold": False}
    return {
        "sam 1024 default": _sam(1024),
        "sam 1024 nofold": _sam(1024, attrs=nofold),
        "sam 1024 nofold norows nocs": _sam(1024, attrs={"norm_fold": False, "attn_rows": False, "win_fused_cs": False}),
        "sam 1024 planes": _sam(1024, ctor={"precise": PRECISE_WIDE_PLANES}),
        "sam 1024 planes norows": _sam(1024, ctor={"precise": PRECISE_WIDE_PLANES}, attrs={"attn_rows": False}),
        "sam 1024 imprecise": _sam(1024, ctor={"precise": ()}),
        "sam 1024 bf16": _sam(1024, ctor={"dtype": torch.bfloat16}),
        "sam 1024 no neck": _sam(1024, use_vit_sam_neck=False, image_embed_dim=768),
        "sam 1024 last block": _sam(1024, last=True),
        "sam 1024 last block nofold": _sam(1024, attrs=nofold, last=True),
        "sam 448 default": _sam(448),
        "sam 448 norows": _sam(448, attrs={"attn_rows": False}),
        "sam 256 default": _sam(256),
        "sam 640 window 20": _sam(640, enc="trace_sam_640_w20"),
        "sam_tiny": _sam(224, enc="sam_tiny", image_embed_dim=96),
        "sam_tiny norows": _sam(224, enc="sam_tiny", image_embed_dim=96, attrs={"attn_rows": False}),
        "sam hd80 448": _sam(448, enc="trace_sam_hd80", image_embed_dim=64),
        "hf 224 default": _hf(224),
        "hf 224 nofold": _hf(224, attrs=nofold),
        "hf 224 nofold norows": _hf(224, attrs={"norm_fold": False, "attn_rows": False}),
        "hf 224 fp8": _hf(224, attrs={"attn_fp8": True}),
        "hf 96 default": _hf(96),
        "hf_tiny 240": _hf(240, enc="hf_tiny", dim=128),
        "hf hd32 160": _hf(160, enc="trace_hf_hd32", dim=128),
        "dinov3 fold 192": _vit("dinov3_fold", 192),
        "dinov3 fold 192 nofold": _vit("dinov3_fold", 192, nofold),
        "dinov3 fold 192 nofold norows": _vit("dinov3_fold", 192, {"norm_fold": False, "attn_rows": False}),
        "dinov3 tiny 64": _vit("dinov3_tiny", 64),
        "dinov3 hd32 64": _vit("dinov3_hd32", 64),
        "dinov2 fold 168": _vit("dinov2_fold", 168),
        "dinov2 fold 168 nofold": _vit("dinov2_fold", 168, nofold),
        "dinov2 fold 224": _vit("dinov2_fold", 224),
        "dinov2 tiny 70": _vit("dinov2_tiny", 70),
        "dinov2 tiny 42": _vit("dinov2_tiny", 42),
        "dinov2 hd32 70": _vit("dinov2_hd32", 70),
    }


def engine(row: dict):
    """The engine of one row, built on the CPU (call under a patched ``_lib``)."""
    from labelanything_amd.engine import LamEngine
    from labelanything_amd.weights import init_state_dict
    _specs()
    cfg = LamConfig(**{"spatial_convs": 3, "custom_preprocess": False, **row["cfg"]})
    eng = LamEngine(cfg, init_state_dict(cfg, 0), torch.device("cpu"), **row["ctor"])
    for k, v in row["attrs"].items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    return eng


def trace(row: dict, setattr_=setattr) -> Recorder:
    """Run one row's encoder under a fresh recorder."""
    rec = Recorder()
    rec.patch(setattr_)
    eng = engine(row)
    s = row["cfg"]["image_size"]
    images = torch.zeros(2, 3, s, s)
    out = eng.sam_encoder(images, want_last_block=True) if row["last"] else eng.encode_images(images)
    rec.note("return", [("", out)])          # which buffers the caller gets
    return rec


def train_matrix() -> dict:
    """name -> configuration of one training-graph row.  Two images each, the smallest shape that reaches the row's path; see the
    module docstring of tests/test_encoder_trace_cpu.py."""
    fused, unfused = {"gemm_fused_act_ok": True}, {"gemm_fused_act_ok": False}

    def row(base: dict, returns=None, dtype=torch.float16, reverse=False, relpos=False, **attrs) -> dict:
        return dict(cfg=base["cfg"], returns=returns, dtype=dtype, reverse=reverse, relpos=relpos, attrs=attrs)

    hf_tiny, sam_tiny = dict(enc="hf_tiny", dim=128), dict(enc="sam_tiny", image_embed_dim=96)
    return {
        "train hf_tiny 240": row(_hf(240, **hf_tiny)),
        "train hf_tiny 224": row(_hf(224, **hf_tiny)),
        "train hf 224 fused act": row(_hf(224), fused),
        "train hf 224 unfused act": row(_hf(224), unfused),
        "train hf 224 exact wgrad": row(_hf(224), fused, fast_wgrad=False),
        "train hf 224 no tn16": row(_hf(224), fused, tn16=False),
        "train hf 224 no fused gelu": row(_hf(224), fused, fused_gelu=False),
        "train hf 224 reversed slots": row(_hf(224), fused, reverse=True),
        "train hf hd32 160": row(_hf(160, enc="trace_hf_hd32", dim=128)),
        "train hf 224 bf16": row(_hf(224), fused, dtype=torch.bfloat16),
        "train sam_tiny": row(_sam(224, **sam_tiny)),
        "train sam_tiny resampled rel-pos": row(_sam(224, **sam_tiny), relpos=True),
        "train sam 448 fused act": row(_sam(448), fused),
        "train sam 448 unfused act": row(_sam(448), unfused),
        "train sam hd80 448": row(_sam(448, enc="trace_sam_hd80", image_embed_dim=64)),
    }


def train_graph(row: dict):
    """The training graph of one row on the CPU (call under a patched ``_lib``), its gradient slots views of ONE flat fp32 buffer in
    ``named_parameters`` order as FlatAdamW packs them.  reverse: laid out AND handed to the graph back to front - the graph's scratch
    follows the order it is given the slots in, and ``_qkv_wgrad_fused`` decides from the distances between the scratch views: query, key
    and value then sit a negative stride apart, and one product per tensor runs."""
    from labelanything_amd.models import Lam
    from labelanything_amd import train_encoder as TE
    _specs()
    cfg = LamConfig(spatial_convs=3, custom_preprocess=False, **row["cfg"])
    lam = Lam(cfg, seed=0, compute_dtype=row["dtype"])
    if row["relpos"]:           # tables of another grid: longer ones for the window block, shorter ones for the global block
        for k, v in [(k, v) for k, v in lam.named_parameters() if "rel_pos" in k]:
            mod, leaf = k.rsplit(".", 1)
            setattr(lam.get_submodule(mod), leaf, torch.nn.Parameter(torch.zeros(v.shape[0] + (8 if ".blocks.0." in k else -6), v.shape[1])))
    named = [(k, p) for k, p in lam.named_parameters() if k.startswith("image_encoder.")]
    flat = torch.zeros(sum(p.numel() for _, p in named))
    views, off = {}, 0
    for k, p in (reversed(named) if row["reverse"] else named):
        views[k] = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    cls = getattr(TE, encoder_kind(cfg.encoder_spec.kind).train_graph)
    # (numerics as LamTrainer chooses them: no token-mean corrections in the saved-activation forward)
    graph = cls(lam, views, precise=tuple(g for g in lam.precise if g not in ("vmean", "projmean")))
    for k, v in row["attrs"].items():
        assert hasattr(graph, k), k
        setattr(graph, k, v)
    return graph


def train_trace(row: dict, setattr_=setattr) -> Recorder:
    """Forward, then backward of an all-ones gradient, of one training row under a fresh recorder.  ``torch.empty`` is ``torch.zeros``
    meanwhile: the host reads a few buffers back (the finite check of the loss-scale loop), which must not see what a recycled
    allocation holds."""
    rec = Recorder(row["returns"])
    rec.patch(setattr_)
    setattr_(torch, "empty", torch.zeros)
    setattr_(torch, "empty_like", torch.zeros_like)
    graph = train_graph(row)
    s = row["cfg"]["image_size"]
    out = graph.forward(torch.zeros(2, 3, s, s))
    rec.note("return", [("", out)])
    graph.backward(torch.ones_like(out))
    return rec


def decoder_matrix() -> dict:
    """name -> configuration of one decoder row: one episode of ``m`` supports and ``c`` classes on a 4 x 4 grid (16 stream rows a slab),
    2 points, 1 box and 16 x 16 masks a (support, class) pair - ``prompts`` says which kinds are passed.  The encoder (sam_tiny) is built
    and never run.  See the module docstring of tests/test_encoder_trace_cpu.py for what each row reaches."""
    def row(d=256, prompts="pbm", m=2, c=3, ctor=None, attrs=None, split_ok=True, **cfg) -> dict:
        returns = {"conv3x3_split_ok": split_ok, "stream_mlp_ok": True, "extract_pool_plan": (64, 2, 4096)}
        cfg = dict(encoder="sam_tiny", image_size=64, image_embed_dim=96, embed_dim=d, **cfg)
        return dict(cfg=cfg, ctor=ctor or {}, attrs=attrs or {}, returns=returns, prompts=prompts, m=m, c=c)

    def bank(d):
        return {"name": "RandomMatrixEncoder", "bank_size": 10, "embed_dim": d}

    f16x2, one_way, pool = {"decoder_dtype": "f16x2"}, {"fusion_transformer": "OneWayTransformer"}, {"prompt_encoder": "TokenPool"}
    return {
        "dec 64 all prompts": row(64),
        "dec 64 points": row(64, "p"),
        "dec 64 boxes": row(64, "b"),
        "dec 64 masks": row(64, "m"),
        "dec 64 merge attentions bank": row(64, class_attention=True, example_attention=True, example_class_attention=True,
                                            class_encoder=bank(64)),
        "dec 256 fused": row(),
        "dec 256 f16x2": row(ctor=f16x2),
        "dec 256 f16x2 unfused": row(ctor={"fuse_twoway": False, **f16x2}),
        "dec 256 16-bit im2col": row(ctor={"decoder_dtype": None}),
        "dec 256 unfused": row(ctor={"fuse_twoway": False}),
        "dec 256 conv_split off": row(attrs={"conv_split": False}),
        "dec 256 33 classes": row(c=33),
        "dec 256 no spatial convs": row(spatial_convs=0),
        "dec oneway fused chain mlp": row(**one_way),
        "dec oneway fused stream_mlp": row(attrs={"ONEWAY_MLP_MIN_ROWS": 0}, **one_way),
        "dec oneway unfused": row(ctor={"fuse_oneway": False}, **one_way),
        "dec oneway f16x2": row(ctor=f16x2, **one_way),
        "dec oneway f16x2 unfused": row(ctor={"fuse_oneway": False, **f16x2}, **one_way),
        "dec pool masks": row(prompts="pbm", **pool),
        "dec pool no masks": row(prompts="pb", **pool),
        "dec pool masks only": row(prompts="m", **pool),
        "dec pool 36 tokens bank": row(prompts="pbm", c=9, class_encoder=bank(256), **pool),
        "dec cross_attention 2 queries": row(embedding_extraction="cross_attention", embeddings_per_example=2, segment_example_logits=True),
        "dec cross_attention 16-bit": row(ctor={"decoder_dtype": None}, embedding_extraction="cross_attention", embeddings_per_example=2,
                                          segment_example_logits=True),
        "dec 4 embeddings per example": row(embeddings_per_example=4, segment_example_logits=True),
        "dec two levels": row(classification_levels=2),
        "dec conv classification": row(conv_classification=True),
        "dec downsample rate 1": row(classification_layer_downsample_rate=1, split_ok=False),
    }


def _tensors(prefix: str, v):
    """(name, tensor) of every tensor in a result: a dictionary, a tuple or a tensor."""
    if isinstance(v, torch.Tensor):
        yield prefix, v
    elif isinstance(v, dict):
        for k in sorted(v):
            yield from _tensors(f"{prefix}.{k}" if prefix else k, v[k])
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            yield from _tensors(f"{prefix}[{i}]", x)


def decoder_trace(row: dict, setattr_=setattr) -> Recorder:
    """Prompt encoder, mask decoder and post-processing of one decoder row under a fresh recorder, called as ``Lam._run`` calls them.
    ``Tensor.pin_memory`` is an identity meanwhile (``LamEngine.h2d`` pins, which needs a GPU) and ``selected_rows`` is always passed
    (``sample_rows`` draws a permutation).  The last line holds every tensor of the prompt encoder's result and of the output: which
    are arena views, which clones."""
    rec = Recorder(row["returns"])
    rec.patch(setattr_)
    setattr_(torch.Tensor, "pin_memory", lambda t, *a, **k: t)
    eng = engine(row)
    cfg = eng.cfg
    b, m, c, g, d, s = 1, row["m"], row["c"], 4, cfg.embed_dim, cfg.image_size
    z = torch.zeros
    points = (z(b, m, c, 2, 2), z(b, m, c, 2, dtype=torch.int32)) if "p" in row["prompts"] else None
    boxes = (z(b, m, c, 1, 4), z(b, m, c, 1, dtype=torch.int32)) if "b" in row["prompts"] else None
    masks = (z(b, m, c, 4 * g, 4 * g), z(b, m, c, dtype=torch.int32)) if "m" in row["prompts"] else None
    flag_examples = z(b, m, c, dtype=torch.uint8)
    res = eng.prompt_encoder(z(b * m * g * g, d), b, m, g, points, boxes, masks, flag_examples, torch.arange(c))
    seg = eng.mask_decoder(z(b * g * g, d), b, g, res.get("class_embeddings"), res["class_examples_embeddings"], res["flag_examples"])
    fg = eng.example_valid(res["flag_examples"]) if cfg.segment_example_logits else None
    out = eng.postprocess_dev(seg, torch.tensor([[s, s, s, s]] * b, dtype=torch.int32), s, s, fg, True)
    rec.note("return", list(_tensors("", {"prompt_encoder": res, "low_res_logits": seg, "post": out})))
    return rec


def _sha_entries(key: str, v):
    if isinstance(v, torch.Tensor):
        raw = v.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        yield key, tuple(v.shape), str(v.dtype)[6:], hashlib.sha256(raw).hexdigest()
    else:
        for i, x in enumerate(v):
            yield from _sha_entries(f"{key}[{i}]", x)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--print", dest="show", metavar="NAME")
    g.add_argument("--table", action="store_true")
    g.add_argument("--train-table", action="store_true")
    g.add_argument("--decoder-table", action="store_true")
    g.add_argument("--packed", metavar="NAME")
    a = ap.parse_args()
    rows = matrix()
    if a.table:
        for name, row in rows.items():
            n, h = trace(row).digest()
            print(f"{name!r}: ({n}, {h!r}),")
    elif a.train_table or a.decoder_table:
        for name, row in (train_matrix() if a.train_table else decoder_matrix()).items():
            rec = train_trace(row) if a.train_table else decoder_trace(row)
            n, h = rec.digest()
            print(f"{name!r}: ({n}, {h!r},\n{'':{len(name) + 9}}{rec.digest(shape=True)[1]!r}),")
    elif a.show in train_matrix():
        print("\n".join(train_trace(train_matrix()[a.show]).lines))
    elif a.show in decoder_matrix():
        print("\n".join(decoder_trace(decoder_matrix()[a.show]).lines))
    elif a.show:
        print("\n".join(trace(rows[a.show]).lines))
    else:
        Recorder().patch(setattr)
        eng = engine(rows[a.packed])
        for k, v in sorted(eng.p.items()) + sorted((k, v) for k, v in eng.w32.items() if k.startswith("image_encoder.")):
            for ent in _sha_entries(k, v):
                print(*ent)


if __name__ == "__main__":
    main()
