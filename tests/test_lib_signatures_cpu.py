"""CPU: the binding's signature table and struct mirrors against include/la_hip.h, and the one call path's refusal of host tensors.

The header is the contract; ``_lib.SIGNATURES`` restates it one line per entry point (``lib()`` sets every ``argtypes`` from it) and five
``ctypes.Structure`` classes restate its structs.  Both are compared here position by position, so a parameter or field added on one side
fails a test instead of shifting what follows it.
"""
import ctypes as C
import os
import re

import pytest
import torch

from labelanything_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {("int",): "i", ("long",): "l", ("long", "long"): "q", ("float",): "f"}
STRUCTS = ("LaGemmEpilogue", "LaGemmPlan", "LaAttnCall", "LaAttnLaunch", "LaAttnPlan")


def header() -> str:
    with open(os.path.join(ROOT, "include", "la_hip.h")) as fh:
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S))


def kind(decl: str) -> str:
    """'*' for any pointer, else the table's letter of the scalar type in front of the parameter's name."""
    if "*" in decl:
        return "*"
    return SCALARS[tuple(w for w in decl.split()[:-1] if w != "const")]          # KeyError: a kind the binding has no letter for


def prototypes():
    """name -> (kinds per position, last parameter is ``void* stream``) for every ``la_*`` prototype of the header."""
    out = {}
    for name, params in re.findall(r"^\s*(?:int|const\s+char\s*\*)\s+(la_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header(), flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        if params == ["void"]:
            params = []
        assert name not in out, f"{name} declared twice"
        out[name] = ("".join(kind(p) for p in params), bool(params) and params[-1] == "void* stream")
    return out


def struct_fields(name: str):
    """[(field, kind)] of ``typedef struct name { ... } name;`` in declaration order; kind as ``kind()``, or the element type and length of
    an array of structs."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header(), flags=re.S).group(1)
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        first, *more = decl.split(",")
        base, first = first.rsplit(" ", 1) if "*" not in first else (first[:first.index("*")], first[first.index("*"):])
        for d in [first] + more:
            d = d.strip()
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", d)
            if arr:
                fields.append((arr.group(1), (base.strip(), int(arr.group(2)))))
            else:
                fields.append((d.lstrip("* "), "*" if d.startswith("*") else kind(base + " x")))
    return fields


def test_table_and_header_declare_the_same_entry_points_with_the_same_parameters():
    protos = prototypes()
    assert len(protos) == len(_lib.EXPORTS) + 2, "a prototype of include/la_hip.h was not read (or EXPORTS lost an entry)"
    assert protos.pop("la_last_error") == ("", False) and protos.pop("la_version") == ("", False)
    assert sorted(protos) == sorted(_lib.SIGNATURES) and _lib.EXPORTS == list(_lib.SIGNATURES)
    for name, (kinds, streamed) in protos.items():
        sig = _lib.SIGNATURES[name]
        assert set(sig) <= set("phsilqf"), name
        assert re.sub("[phs]", "*", sig) == kinds, f"{name}: table {sig} against header {kinds}"
        assert ("s" in sig, sig.endswith("s"), sig.count("s") <= 1) == (streamed, streamed, True), f"{name}: the stream is the last parameter or absent"


def test_loaded_library_is_typed_from_the_table():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.lib()
    ctype = {"p": C.c_void_p, "h": C.c_void_p, "s": C.c_void_p, "i": C.c_int, "l": C.c_long, "q": C.c_longlong, "f": C.c_float}
    for name, sig in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [ctype[k] for k in sig], name
    # a `long` count travels whole: 2^32 pixels cut to a C int would be HW = 0, which the library refuses
    assert _lib.logits_objective_workspace_bytes(1, 2, 1 << 32) > 0
    assert _lib.extract_pool_plan(2, 4096, 256, 8)[2] > 0
    with pytest.raises(C.ArgumentError):                            # only a device-pointer position takes a tensor
        _lib._call(lib.la_logits_objective_workspace_bytes, 1, 2, 16, torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("name", STRUCTS)
def test_struct_mirror_has_the_headers_fields(name):
    mirror = getattr(_lib, name)._fields_
    declared = struct_fields(name)
    assert [f for f, _ in mirror] == [f for f, _ in declared]
    for (field, ctype), (_, k) in zip(mirror, declared):
        if isinstance(k, tuple):
            assert issubclass(ctype, C.Array) and ctype._type_ is getattr(_lib, k[0]) and ctype._length_ == k[1], field
        else:
            assert ctype is {"*": C.c_void_p, "i": C.c_int}[k], field


class CountingLibrary:
    """Stands in for the loaded library: every symbol is a function that counts its calls (none may happen)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        fn.__name__ = name
        return fn


def host_calls():
    """(wrapper, arguments) with small HOST tensors that pass the wrapper's own shape / dtype validation: the wrappers that had no device
    check of their own, one that checked its first tensor only (the host tensor comes later), and the tensors that travel inside
    ``gemm``'s epilogue struct and ``mask_embed``'s weight list."""
    L = _lib
    f32, f16 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.float16))
    i64, u8, i32 = (lambda *s: torch.zeros(*s, dtype=torch.int64)), (lambda *s: torch.zeros(*s, dtype=torch.uint8)), \
        (lambda *s: torch.zeros(*s, dtype=torch.int32))
    w12 = [f32(4) for _ in range(12)]
    return [
        (L.relpos_terms, (f16(4, 192), 1, 1, 2, 64, f16(3, 64), f16(3, 64), f32(1, 4, 2), f32(1, 4, 2))),
        (L.attn_fwd, (f16(4, 192), f16(64, 64), f16(4, 64), None, None, 1, 1, 4, 64, 2, 64, 0.125, L.ATTN_PLAIN)),
        (L.attn_fwd_cs, (f16(4, 192), f16(64, 64), f16(4, 64), None, None, 1, 1, 4, 64, 2, 64, 0.125, L.ATTN_PLAIN, f32(1, 64))),
        (L.colmean, (f32(2, 4, 8), 2, 4, 8, f32(2, 8), f32(2, L.COLMEAN_SPLIT, 8))),
        (L.class_mean, (f32(1, 2, 2, 8), u8(1, 2, 2), 1, 2, 2, 8, f32(1, 2, 8))),
        (L.classify, (f32(1, 4, 8), f32(1, 2, 8), 1, 4, 2, 8, f32(1, 2, 4))),
        (L.post_final, (f32(1, 2, 8, 8), 1, 2, 8, i32(1, 4), None, 4, 4, f32(1, 2, 4, 4), i64(1, 4, 4))),
        (L.error_count, (f32(1, 2, 4, 4), i64(1, 4, 4), 1, 2, 4, 4, -100, i32(1, 2, 1))),
        (L.error_points, (f32(1, 2, 4, 4), i64(1, 4, 4), 1, 2, 4, 4, -100, i32(1, 2, 1), 1, None, f32(1, 2, 1), None, 0, 8, False,
                          f32(1, 2, 1, 2), f32(1, 2, 1))),
        (L.attn_small_lse, (f32(4, 8), f32(4, 8), 1, 4, 4, 2, 4, f32(4, 2))),
        (L.attn_small_bwd, (f32(4, 8), f32(4, 8), f32(4, 8), None, f32(4, 8), None, 1, 4, 4, 2, 4, f32(4, 8), f32(4, 8), f32(4, 8))),
        (L.mask_embed, (None, None, 1, 1, 8, 2, 4, w12, None, None, f32(4, 4), f32(4, 4), None, None, L.LA_F32)),
        (L.mask_embed_pooled, (None, None, 1, 1, 8, 2, 4, w12, None, None, f32(4, 4), f32(4, 4), None, None, L.LA_F32)),
    ]


@pytest.mark.parametrize("wrapper,args", host_calls(), ids=lambda v: getattr(v, "__name__", ""))
def test_host_tensors_are_refused_before_the_library_is_reached(monkeypatch, wrapper, args):
    fake = CountingLibrary()
    monkeypatch.setattr(_lib, "_lib", fake)
    with pytest.raises(RuntimeError, match="device tensors"):
        wrapper(*args)
    assert fake.calls == []


def test_tensors_that_travel_inside_a_struct_are_checked_by_gemm_and_not_by_gemm_plan(monkeypatch):
    """``_call(..., also=...)`` holds the tensors a call reaches through its epilogue struct to the arguments' rule.  The device operands
    are stood in for by plain addresses, which the call path never checks - that is what lets ``gemm_plan`` run without a GPU."""
    fake = CountingLibrary()
    monkeypatch.setattr(_lib, "_lib", fake)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: type("Stream", (), {"cuda_stream": 0})())
    host = torch.zeros(8, 8, dtype=torch.float16)
    _lib._call(fake.la_gemm, 256, 64, 512, 64, 8, 8, 64, None, _lib.LA_F16, also=(None, 4096, (0, 0, 0, 0, 0)))
    assert fake.calls == ["la_gemm"]                                # addresses, None and plain values pass
    with pytest.raises(RuntimeError, match="device tensors"):
        _lib._call(fake.la_gemm, 256, 64, 512, 64, 8, 8, 64, None, _lib.LA_F16, also=(None, host))
    _lib.gemm_plan(256, 64, 512, 64, 8, 8, 64, _lib.LA_F16, ncu=256, out16=host)
    assert fake.calls == ["la_gemm", "la_gemm_plan"]                # the plan takes any address unchecked
    with pytest.raises(RuntimeError, match="device tensors"):
        _lib.gemm(torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8, 64, dtype=torch.float16), out16=host)
    assert fake.calls == ["la_gemm", "la_gemm_plan"]
