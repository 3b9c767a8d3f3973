"""Score profiles that move the running softmax maximum, and plain fp64 references, for tests/test_softmax_profiles_cpu.py and
tests/test_attention_conditioning_gpu.py.  No kernel code.

The encoder attention kernels (csrc/attn_enc.hip) walk the keys in tiles of 64 and keep an online softmax whose running maximum is
DEFERRED: after tile 0 it advances only when some row of a 32-row wave outgrows it by more than 2^8.  Inputs drawn
from N(0, 1) never do that, so the rescale of l and of the O accumulator after tile 0 is dead code on them.  The builders below make
q | k | v (and rel-pos tables) whose fp64 score matrix S - log2 units, bias included - has stated properties per query row over tiles
of 64 consecutive keys IN THE KERNEL'S KEY ORDER (``tile_of_key``: key // 64, or (kh * 16 + kw) // 64 for the 16-wide slot order of
LA_ATTN_RELPOS_WIN16).  ``check_profile`` measures those properties on S alone and raises when one is missing.

How a profile is realised.  One head dimension c is set aside: q[row, c] = 8 on "loud" rows (even row index) and 0 on "quiet" rows (odd),
k[key, c] = level(key), so a loud row's score is 8 * scale * level(key) nat plus small noise from the other dimensions (q 0.1, k 0.2
N(0, 1): 0.02 nat at hd 64, so that a 9.4 log2 step stays >= 9 on every one of 4096 rows).  Levels are multiples of 1 / 4 with few
bits - exact in fp16, bf16 and e4m3.  Everything is rounded to the operand type before use, so against fp64 only the accumulation
order and the 16-bit rounding of P and O remain.

    stairs   tile 0 flat at 0; ONE key of tile 1 at +step; tile 2 flat at +step; ONE key of tile 3 at +2 step (the rest of it at 0); later
             tiles flat at +step.
             step = 6.5 nat = 9.4 log2: two seams where the tile maximum exceeds everything earlier by >= 9, with >= 2 % of the mass
             through that tile held by the earlier keys.  (Two CONSECUTIVE seams cannot both have that: a rise of 2^9 at a single key
             leaves the earlier 64-key tile at most 64 / 576 of the mass, and the tile after it would need that key's whole tile to
             weigh 2 % of 2^18 - hence the plateau in tile 2.)
    creep    4 keys of tile 1 at +creep (5 .. 7.5 log2: no rescale, P up to 2^7.5 un-normalised), one key of tile 2 at +step: >= 9 above
             tile 0's maximum - the un-advanced m_run - but < 8 above the true running maximum.
    tail     the last valid key, beside the masked slots of a ragged last tile, at +step above every other key.
    front    tile 0 flat at 0, every later key >= 30 log2 below it: exp2 underflows, nothing is ever rescaled.
    offset   stairs plus a second dimension with q = 16 on every row and k = +-ob on every key: every score moves by the same
             +-(>= 64) log2 units; the output is unchanged and lse moves by exactly that.
    bias     (rel-pos) the rise comes from tabh through q . Rh[qy - kh + G - 1]: Rh[i, c] = step / 8 for key rows kh >= qy + K0 (and twice
             that for kh >= qy + K0 + 40), so the seam sits at a different key row - a different tile - for every query row, and for
             G = 64 in the per-tile row term.  k[key, c] only SUPPRESSES (-10 nat): key rows < K0 (tiles 0 .. first seam) are left
             alone, of the later rows every second one keeps one key (column 0) and the rest are pushed down.  A table term shifts WHOLE
             key rows, all query columns alike, so without that suppression the share of the earlier keys at a seam is at most
             rows / (rows + 2^9 rows of the new tile) < 2 % for every G <= 20.  For the same reason a SECOND qualifying seam needs
             >= 18 live key rows on the plateau: G = 64 has them (rows with qy + K0 + 40 < G: 20 live rows, share 2.3 %), the small
             grids cannot.  The stated condition is therefore: every loud row has >= 1 qualifying seam, the seams of the loud rows fall into >= 2 different
             tiles, and with the tables zeroed no row rises by more than 6.
"""
from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
TILE = 64
NEG = -1.0e30

TOL16 = {"f16": 2e-3, "bf16": 1.6e-2}
TOL_LSE = 2e-3
TOL_FP8 = 3e-3
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}

KINDS_PLAIN = ("stairs", "creep", "tail", "front", "offset+", "offset-")
KINDS_RELPOS = ("stairs", "creep", "bias")


def round_to(x: torch.Tensor, dt: str) -> torch.Tensor:
    """fp64 tensor holding exactly the values the operand type ``dt`` can hold."""
    if dt == "e4m3":
        return x.float().to(torch.float8_e4m3fn).double()
    return x.to(TORCH_DT[dt]).double()


def tiles_linear(t: int) -> torch.Tensor:
    return torch.arange(t) // TILE


def tiles_win16(g: int) -> torch.Tensor:
    """key kh * g + kw -> tile of slot kh * 16 + kw."""
    key = torch.arange(g * g)
    return ((key // g) * 16 + key % g) // TILE


def tile_map(order: str, t: int, g: int = 0) -> torch.Tensor:
    return tiles_win16(g) if order == "win16" else tiles_linear(t)


def profile_channel(hd: int):
    """(profile dimension, offset dimension): for hd 128 the profile dimension is in the upper 64 columns, the offset one in the lower."""
    return (hd - 64 + 5, 41)


def _levels(kind: str, tile_of_key: torch.Tensor, unit_nat: float) -> torch.Tensor:
    """k[key, c] of the plain profiles; a loud row's score is unit_nat * level nat."""
    t = tile_of_key.numel()
    step = math.ceil(6.5 / unit_nat * 4.0) / 4.0               # 6.5 (hd 64: 9.38 log2) and 9.25 (hd 128: 9.44 log2): exact in e4m3 / bf16
    creep = round(4.2 / unit_nat)
    lvl = torch.zeros(t, dtype=torch.float64)

    def pick(j, n=1):
        keys = torch.nonzero(tile_of_key == j).flatten()
        first = (keys.numel() * 37) // TILE
        return keys[first:first + n]

    if kind in ("stairs", "offset+", "offset-"):
        lvl[tile_of_key == 2] = step
        lvl[tile_of_key >= 4] = step
        lvl[pick(1)] = step
        lvl[pick(3)] = 2 * step
    elif kind == "creep":
        lvl[pick(1, 4)] = creep
        lvl[pick(2)] = step
    elif kind == "tail":
        lvl[t - 1] = step
    elif kind == "front":
        lvl[tile_of_key >= 1] = -math.ceil(22.0 / unit_nat)
    else:
        raise ValueError(kind)
    return lvl


def bias_k0(tile_of_key: torch.Tensor, g: int) -> int:
    """first key row whose column-0 key lies beyond tile 0"""
    return int(min(kh for kh in range(g) if int(tile_of_key[kh * g]) >= 1))


def build(kind: str, t: int, hd: int, dt: str, tile_of_key: torch.Tensor, *, b: int = 2, heads: int = 2, g: int = 0, seed: int = 0) -> dict:
    """-> dict(q, k, v: fp64 [b, heads, t, hd] holding ``dt`` values; scale; loud: bool [t]; tabh, tabw: fp64 [2g - 1, hd] when g > 0).
    The same profile in every (image, head); the noise differs."""
    gen = torch.Generator().manual_seed(1000 * t + 10 * hd + seed)
    scale = 1.0 / math.sqrt(hd)
    unit_nat = 8.0 * scale
    c, c2 = profile_channel(hd)
    q = 0.1 * torch.randn(b, heads, t, hd, generator=gen, dtype=torch.float64)
    k = 0.2 * torch.randn(b, heads, t, hd, generator=gen, dtype=torch.float64)
    v = torch.randn(b, heads, t, hd, generator=gen, dtype=torch.float64)
    loud = (torch.arange(t) % 2) == 0
    q[..., c] = torch.where(loud, 8.0, 0.0)
    out = {"scale": scale, "kind": kind}
    if g:
        tabh = 0.01 * torch.randn(2 * g - 1, hd, generator=gen, dtype=torch.float64)
        tabw = 0.01 * torch.randn(2 * g - 1, hd, generator=gen, dtype=torch.float64)
        tabh[:, [c, c2]] = 0.0
        tabw[:, [c, c2]] = 0.0
    if kind == "bias":
        assert g > 0
        k0 = bias_k0(tile_of_key, g)
        kh, kw = torch.arange(t) // g, torch.arange(t) % g
        live = (kh < k0) | (((kh - k0) % 2 == 0) & (kw == 0))
        k[..., c] = torch.where(live, 0.0, -float(math.ceil(10.0 / unit_nat)))
        d = torch.arange(2 * g - 1) - (g - 1)                        # qy - kh of table row i
        tabh[:, c] = 0.84375 * ((d <= -k0).double() + (d <= -k0 - 40).double())       # 8 * 0.84375 = 6.75 nat = 9.74 log2 a step
        qy = torch.arange(t) // g
        loud = loud & (qy + k0 + qy % 2 <= g - 1)                    # (the first key row past the step that kept its key)
        q[..., c] = torch.where((torch.arange(t) % 2) == 0, 8.0, 0.0)
    else:
        lvl = _levels(kind, tile_of_key, unit_nat)
        k[..., c] = lvl
        if kind in ("stairs", "offset+", "offset-"):
            # V with a contrast between the spike keys and the keys before them: a fault that merely drops or overweighs the earlier
            # state (P against the stale maximum) moves the output by (earlier share) x (contrast), and the share cannot exceed
            # 64 / (64 + 2^9) at a single-key seam - with plain N(0, 1) values that is below 10 x the bf16 bound.
            spike = torch.zeros(t, dtype=torch.bool)
            for j in (1, 3):
                sel = tile_of_key == j
                spike |= sel & (lvl == lvl[sel].max())
            pattern = torch.where(torch.rand(b, heads, 1, hd, generator=gen) < 0.5, -4.0, 4.0).double()
            v = 0.125 * v + pattern * torch.where(spike, -1.0, 1.0)[:, None]
        if kind.startswith("offset"):
            ob = math.ceil(64.0 / (16.0 * scale * LOG2E) * 4.0) / 4.0
            if dt == "e4m3":
                ob = 24.0                                            # (22.25 needs 7 bits; 16 x 24 / 8 = 69.2 log2)
            q[..., c2] = 16.0
            k[..., c2] = ob if kind == "offset+" else -ob
            out["offset_log2"] = (16.0 * ob * scale * LOG2E) * (1.0 if kind == "offset+" else -1.0)
    out.update(q=round_to(q, dt), k=round_to(k, dt), v=round_to(v, "f16" if dt == "e4m3" else dt), loud=loud)
    if g:
        out.update(tabh=round_to(tabh, dt), tabw=round_to(tabw, dt), g=g)
    return out


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------
def relpos_terms(q, tabh, tabw, g):
    """q [b, heads, g * g, hd], tables [2g - 1, hd] -> (relh, relw) [b * heads, t, g]: q . Rh[qy - kh + g - 1], q . Rw[qx - kw + g - 1]
    (the decomposed relative position terms, as _relpos_reference of tests/test_sam_train_gpu.py)."""
    b, heads, t, hd = q.shape
    idx = (torch.arange(g)[:, None] - torch.arange(g)[None, :] + (g - 1)).to(q.device)
    r_q = q.reshape(b * heads, g, g, hd)
    rel_h = torch.einsum("bhwc,hkc->bhwk", r_q, tabh[idx])
    rel_w = torch.einsum("bhwc,wkc->bhwk", r_q, tabw[idx])
    return rel_h.reshape(b * heads, t, g), rel_w.reshape(b * heads, t, g)


def scores_nat(q, k, scale, g=0, tabh=None, tabw=None):
    """[b, heads, t, t] logits (nat), rel-pos bias included when g > 0."""
    s = (q * scale) @ k.transpose(-1, -2)
    if g:
        b, heads, t, _ = q.shape
        rel_h, rel_w = relpos_terms(q, tabh, tabw, g)
        s = (s.view(b * heads, t, g, g) + rel_h[..., :, None] + rel_w[..., None, :]).view(b, heads, t, t)
    return s


def scores_log2(p: dict, tables: bool = True) -> torch.Tensor:
    g = p.get("g", 0)
    if g and not tables:
        z = torch.zeros_like(p["tabh"])
        return scores_nat(p["q"], p["k"], p["scale"], g, z, z) * LOG2E
    return scores_nat(p["q"], p["k"], p["scale"], g, p.get("tabh"), p.get("tabw")) * LOG2E


def attention(q, k, v, scale, g=0, tabh=None, tabw=None):
    """-> (O [b, heads, t, hd], lse [b, heads, t] in log2 units); differentiable."""
    s = scores_nat(q, k, scale, g, tabh, tabw)
    return torch.softmax(s, -1) @ v, torch.logsumexp(s, -1) * LOG2E


def rows_of(x):
    """[b, heads, t, hd] -> [b * t, heads * hd]"""
    b, heads, t, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * t, heads * hd)


def pack_qkv(p: dict, dtype, device="cpu"):
    """-> qkv [b * t, 3 E] rows (q | k | v, head-major columns) in ``dtype``."""
    return torch.cat([rows_of(p["q"]), rows_of(p["k"]), rows_of(p["v"])], dim=1).to(dtype).to(device).contiguous()


# ---- the profile conditions, measured on S -------------------------------------------------------------------------------------------
def seam_stats(s2: torch.Tensor, tile_of_key: torch.Tensor):
    """s2 [rows, keys] log2.  -> (tmax [rows, ntiles], rise [rows, ntiles]: tile maximum minus the maximum over all earlier tiles
    (tile 0: 0), share [rows, ntiles]: softmax mass of the earlier keys / mass through the tile)."""
    nt = int(tile_of_key.max()) + 1
    rows = s2.shape[0]
    ref = s2.max(1, keepdim=True).values
    w = torch.exp2(s2 - ref)
    tmax = torch.stack([s2[:, tile_of_key == j].max(1).values for j in range(nt)], 1)
    mass = torch.stack([w[:, tile_of_key == j].sum(1) for j in range(nt)], 1)
    cum = mass.cumsum(1)
    before = torch.cat([torch.full((rows, 1), NEG, dtype=s2.dtype), tmax.cummax(1).values[:, :-1]], 1)
    rise = tmax - before
    rise[:, 0] = 0.0
    share = (cum - mass) / cum
    return tmax, rise, share


def check_profile(s2: torch.Tensor, tile_of_key: torch.Tensor, kind: str, loud: torch.Tensor = None, s2_base: torch.Tensor = None) -> dict:
    """s2: [rows, keys] fp64 reference scores of ONE (image, head), log2 units, bias included.  loud: bool [rows] (default: even rows).
    s2_base: 'offset': the scores of the same input without the offset dimension; 'bias': the scores with the tables zeroed.
    Returns the measured figures; raises AssertionError when the profile's conditions do not hold."""
    rows = s2.shape[0]
    tile_of_key = tile_of_key.to(s2.device)
    if loud is None:
        loud = (torch.arange(rows) % 2) == 0
    loud = loud.to(s2.device)
    quiet = (torch.arange(rows, device=s2.device) % 2) == 1
    tmax, rise, share = seam_stats(s2, tile_of_key)
    nt = tmax.shape[1]
    out = {"ntiles": nt}
    # both kinds of row in every 32-row wave that holds a loud one (the branch is wave-uniform)
    for w0 in range(0, rows, 32):
        if bool(loud[w0:w0 + 32].any()) and rows - w0 > 1:
            assert bool(quiet[w0:w0 + 32].any()), f"wave at row {w0} holds no quiet row"
    if kind in ("stairs", "offset+", "offset-", "bias"):
        ok = (rise >= 9.0) & (share >= 0.02)
        ok[:, 0] = False
        n_ok = ok[loud].sum(1)
        need = 1 if kind == "bias" else 2
        assert int(n_ok.min()) >= need, f"{kind}: a loud row has {int(n_ok.min())} qualifying seams, {need} needed"
        qr = rise[quiet][:, 1:].max() if kind != "bias" else torch.tensor(0.0)
        assert float(qr) <= 6.0, f"{kind}: a quiet row rises by {float(qr):.2f}"
        out.update(min_rise=float(rise[loud][ok[loud]].min()), min_share=float(share[loud][ok[loud]].min()), quiet_rise=float(qr),
                   seams_min=int(n_ok.min()), seams_max=int(n_ok.max()), rows_two_seams=int((n_ok >= 2).sum()))
        if kind == "bias":
            seam_tiles = torch.nonzero(ok[loud].any(0)).flatten().tolist()
            assert len(seam_tiles) >= 2, f"bias: the seams of all loud rows fall into tiles {seam_tiles}"
            _, rise0, _ = seam_stats(s2_base, tile_of_key)
            assert float(rise0[:, 1:].max()) <= 6.0, "bias: a rise that does not come from the tables"
            qr = rise[quiet][:, 1:].max()
            assert float(qr) <= 6.0, f"bias: a quiet row rises by {float(qr):.2f}"
            out.update(seam_tiles=seam_tiles, quiet_rise=float(qr))
        if kind.startswith("offset"):
            d = s2 - s2_base
            assert float((d - d[0, 0]).abs().max()) <= 1e-9 and abs(float(d[0, 0])) >= 64.0, "offset: not one common shift of >= 64"
            out["offset"] = float(d[0, 0])
    elif kind == "creep":
        lo = rise[loud]
        sh = share[loud]
        first = ((lo >= 5.0) & (lo <= 7.5) & (sh >= 0.10))
        first[:, 0] = False
        above0 = tmax[loud] - tmax[loud][:, :1]
        late = torch.zeros_like(first)
        for j in range(2, nt):
            late[:, j] = first[:, 1:j].any(1) & (above0[:, j] >= 9.0) & (lo[:, j] < 8.0) & (lo[:, j] > 0.0)
        assert bool(first.any(1).all()), "creep: a loud row has no seam with a rise in [5, 7.5] and >= 10 % earlier mass"
        assert bool(late.any(1).all()), "creep: a loud row has no later tile >= 9 above tile 0 and < 8 above the running maximum"
        assert float(rise[quiet][:, 1:].max()) <= 6.0
        out.update(creep_rise=float(lo[first].min()), creep_share=float(sh[first].min()), late_above_tile0=float(above0[late].min()),
                   late_rise=float(lo[late].max()))
    elif kind == "tail":
        last = s2.shape[1] - 1
        assert int((tile_of_key == nt - 1).sum()) < TILE, "tail: the last tile is not ragged"
        assert int(tile_of_key[last]) == nt - 1
        gap = s2[loud][:, last] - s2[loud][:, :last].max(1).values
        assert float(gap.min()) >= 9.0, f"tail: the last key is only {float(gap.min()):.2f} above the others"
        out.update(tail_gap=float(gap.min()), tail_share=float(share[loud][:, nt - 1].min()))
    elif kind == "front":
        k0 = tile_of_key == 0
        gap = s2[loud][:, k0].max(1).values - s2[loud][:, ~k0].max(1).values
        assert float(gap.min()) >= 30.0, f"front: a later key is only {float(gap.min()):.2f} below tile 0"
        assert float(rise[quiet][:, 1:].max()) <= 6.0
        out.update(front_gap=float(gap.min()))
    else:
        raise ValueError(kind)
    return out


def check_built(p: dict, tile_of_key: torch.Tensor) -> dict:
    """check_profile on (image 0, head 0) and on the last (image, head) of a built input."""
    kind = p["kind"]
    s2 = scores_log2(p)
    base = None
    if kind.startswith("offset"):
        c2 = profile_channel(p["q"].shape[-1])[1]
        p0 = dict(p, q=p["q"].clone())
        p0["q"][..., c2] = 0.0
        base = scores_log2(p0)
    elif kind == "bias":
        base = scores_log2(p, tables=False)
    out = None
    for bi, hi in {(0, 0), (s2.shape[0] - 1, s2.shape[1] - 1)}:
        out = check_profile(s2[bi, hi], tile_of_key, kind, p["loud"], None if base is None else base[bi, hi])
    return out


# ---- a torch model of the kernels' softmax policy ------------------------------------------------------------------------------------
FAULTS = ("no_o_rescale", "no_l_rescale", "stale_max", "half_o_rescale")


def kernel_order(s2: torch.Tensor, v: torch.Tensor, order: str, g: int = 0):
    """scores [rows, keys] and V [keys, hd] in the kernel's key order, padded to whole tiles with masked (NEG) slots."""
    t = s2.shape[1]
    if order == "win16":
        slots = -(-16 * g // TILE) * TILE
        key = torch.arange(t)
        slot = (key // g) * 16 + key % g
    else:
        slots = -(-t // TILE) * TILE
        slot = torch.arange(t)
    sp = torch.full((s2.shape[0], slots), NEG, dtype=s2.dtype)
    vp = torch.zeros(slots, v.shape[1], dtype=v.dtype)
    sp[:, slot] = s2
    vp[slot] = v
    return sp, vp


def deferred_softmax_model(sp: torch.Tensor, vp: torch.Tensor, pdt: str, fault: str = None, thr: float = 8.0):
    """Tile-wise online softmax with a deferred maximum: 64-key tiles, 32-row groups; after a group's first tile its running maximum
    advances only when some row of the group outgrows it by more than ``thr`` log2 units, and only then are l and O multiplied by alpha.
    P is rounded to ``pdt`` before P . V (fp64 otherwise).  sp [rows, slots] log2 scores in kernel order (NEG = masked), vp [slots, hd].
    fault: one of FAULTS, applied after tile 0.  -> (O [rows, hd], lse [rows] log2, number of rescales after tile 0)."""
    rows, hd = sp.shape[0], vp.shape[1]
    o = torch.zeros(rows, hd, dtype=torch.float64)
    l = torch.zeros(rows, dtype=torch.float64)
    m = torch.full((rows,), NEG, dtype=torch.float64)
    fired = 0
    for j in range(sp.shape[1] // TILE):
        s = sp[:, j * TILE:(j + 1) * TILE]
        mx = s.max(1).values
        m_for_p = m.clone()
        for r0 in range(0, rows, 32):
            sl = slice(r0, min(r0 + 32, rows))
            if bool((mx[sl] - m[sl] > thr).any()):
                m_new = torch.maximum(m[sl], mx[sl])
                alpha = torch.exp2(m[sl] - m_new)
                f = fault if j > 0 else None
                fired += j > 0
                if f != "no_l_rescale":
                    l[sl] = l[sl] * alpha
                if f == "half_o_rescale":
                    o[sl, :hd // 2] = o[sl, :hd // 2] * alpha[:, None]
                elif f != "no_o_rescale":
                    o[sl] = o[sl] * alpha[:, None]
                m[sl] = m_new
                m_for_p[sl] = m[sl] if f != "stale_max" else m_for_p[sl]
        p = torch.exp2(s - m_for_p[:, None])
        l = l + p.sum(1)
        o = o + round_to(p, pdt) @ vp[j * TILE:(j + 1) * TILE]
    return o / l[:, None], m + torch.log2(l), int(fired)


# ---- the cases of tests/test_attention_conditioning_gpu.py (the CPU module checks every one of them) ----------------------------------
def forward_cases():
    """(family, kind, t, g, hd, dt, order, b, heads)"""
    cases = []
    for dt in ("f16", "bf16"):
        for hd in (64, 128):
            for t in (200, 256):
                for kind in KINDS_PLAIN:
                    if kind == "tail" and t % TILE == 0:
                        continue
                    cases.append(("plain", kind, t, 0, hd, dt, "linear", 2, 2))
        for kind in KINDS_RELPOS:
            for g in (14, 20):
                cases.append(("terms", kind, g * g, g, 64, dt, "linear", 2, 2))
            for g, hd in ((14, 64), (16, 64), (14, 128)):
                cases.append(("tables", kind, g * g, g, hd, dt, "linear", 2, 2))
            cases.append(("global", kind, 4096, 64, 64, dt, "linear", 1, 1))
        for g in (14, 16):
            for kind in KINDS_PLAIN + ("bias",):
                if kind == "tail" and (16 * g) % TILE == 0:
                    continue
                cases.append(("win16", kind, g * g, g, 64, dt, "win16", 2, 2))
    for kind in KINDS_RELPOS:
        cases.append(("global", kind, 4096, 64, 128, "f16", "linear", 1, 1))
    for kind in KINDS_PLAIN:
        cases.append(("fp8", kind, 200, 0, 64, "e4m3", "linear", 2, 2))
    return cases


def backward_cases():
    """(family, kind, t, g, hd, dt, b, heads): stairs and offset inputs only"""
    cases = []
    for kind in ("stairs", "offset+", "offset-"):
        for hd in (64, 128):
            cases.append(("plain", kind, 200, 0, hd, "f16", 2, 2))
        for g in (14, 20):
            cases.append(("relpos", kind, g * g, g, 64, "f16", 2, 2))
        cases.append(("relpos", kind, 4096, 64, 64, "f16", 1, 1))
    cases.append(("plain", "stairs", 200, 0, 64, "bf16", 2, 2))
    cases.append(("relpos", "stairs", 196, 14, 64, "bf16", 2, 2))
    return cases


def case_id(c):
    fam, kind, t, g, hd, dt = c[:6]
    return f"{fam}-{kind}-{'G%d' % g if g else 'T%d' % t}-hd{hd}-{dt}"


# ---- SAM windows addressed in image order, with a pad row --------------------------------------------------------------------------
def build_image_windows(dt: str, ih: int = 20, iw: int = 27, g: int = 14, heads: int = 2, hd: int = 64, seed: int = 0) -> dict:
    """One ih x iw image cut into g x g windows (the bottom and right ones padded).  Real keys sit at level 0, the pad row's k at +step:
    every PADDED key of a window is a spike >= 9 log2 above the real ones for the loud rows (even token index inside the window), so
    the pad row takes part in the softmax exactly as the reference's pad-after-norm token does.
    -> dict(img: q | k | v fp64 [1, heads, ih * iw, hd]; pad: (q, k, v) fp64 [heads, hd]; win: the explicit windows as a ``build`` dict
    ([windows, heads, g * g, hd]); rows: image row of every window token, -1 for padding [windows, g * g])."""
    gen = torch.Generator().manual_seed(7000 + seed)
    scale = 1.0 / math.sqrt(hd)
    c, _ = profile_channel(hd)
    n = ih * iw
    q = 0.1 * torch.randn(1, heads, n, hd, generator=gen, dtype=torch.float64)
    k = 0.2 * torch.randn(1, heads, n, hd, generator=gen, dtype=torch.float64)
    v = torch.randn(1, heads, n, hd, generator=gen, dtype=torch.float64)
    pad = [0.1 * torch.randn(heads, hd, generator=gen, dtype=torch.float64) for _ in range(2)] + [torch.randn(heads, hd, generator=gen, dtype=torch.float64)]
    y, x = torch.arange(n) // iw, torch.arange(n) % iw
    q[..., c] = torch.where((((y % g) * g + x % g) % 2) == 0, 8.0, 0.0)
    k[..., c] = 0.0
    pad[1][:, c] = float(math.ceil(7.0 / (8.0 * scale)))
    tabh = 0.01 * torch.randn(2 * g - 1, hd, generator=gen, dtype=torch.float64)
    tabw = 0.01 * torch.randn(2 * g - 1, hd, generator=gen, dtype=torch.float64)
    tabh[:, c] = 0.0
    tabw[:, c] = 0.0
    q, k, v = round_to(q, dt), round_to(k, dt), round_to(v, dt)
    pad = [round_to(z, dt) for z in pad]
    nwy, nwx = -(-ih // g), -(-iw // g)
    rows = torch.full((nwy * nwx, g * g), -1, dtype=torch.long)
    for wy in range(nwy):
        for wx in range(nwx):
            yy = wy * g + torch.arange(g)[:, None]
            xx = wx * g + torch.arange(g)[None, :]
            r = torch.where((yy < ih) & (xx < iw), yy * iw + xx, torch.full_like(yy * iw + xx, -1))
            rows[wy * nwx + wx] = r.reshape(-1)
    ins = rows >= 0

    def windows(z, padz):
        w = z[0][:, rows.clamp(min=0)]                              # [heads, windows, t, hd]
        w = torch.where(ins[None, :, :, None], w, padz[:, None, None, :].expand_as(w))
        return w.permute(1, 0, 2, 3).contiguous()

    win = {"q": windows(q, pad[0]), "k": windows(k, pad[1]), "v": windows(v, pad[2]), "scale": scale, "g": g, "kind": "padspike",
           "tabh": round_to(tabh, dt), "tabw": round_to(tabw, dt), "loud": (torch.arange(g * g) % 2) == 0}
    return {"img": (q, k, v), "pad": pad, "win": win, "rows": rows, "scale": scale, "g": g, "ih": ih, "iw": iw}


def check_pad_spike(iw_: dict) -> dict:
    """Every window that has padding: for its loud real rows the padded keys stand >= 9 log2 above every real key."""
    s2 = scores_log2(iw_["win"])
    ins = iw_["rows"] >= 0
    loud = iw_["win"]["loud"]
    gaps, padded = [], 0
    for w in range(ins.shape[0]):
        if bool(ins[w].all()):
            continue
        padded += 1
        sw = s2[w, 0][ins[w] & loud]
        gaps.append(float((sw[:, ~ins[w]].max(1).values - sw[:, ins[w]].max(1).values).min()))
    assert padded >= 2 and min(gaps) >= 9.0, (padded, gaps)
    return {"padded_windows": padded, "pad_gap": min(gaps)}


def backward_rounding_model(q, k, v, dout, scale, dt: str):
    """dq, dk, dv ([b, heads, t, hd]) of plain attention in fp64 arithmetic with only the 16-bit roundings of the flash backward
    (csrc/attn_bwd.hip): O is read back as stored (16 bit) for delta = dO . O, P and dS = P (dP - delta) become 16-bit MFMA operands,
    and the three results are stored in 16 bits.  Everything else - scores, lse, accumulation - is exact.  What this model misses
    against exact fp64 gradients is the share of an error that 16-bit rounding alone explains."""
    p = torch.softmax((q * scale) @ k.transpose(-1, -2), -1)
    o16 = round_to(p @ v, dt)
    ds16 = round_to(p * (dout @ v.transpose(-1, -2) - (dout * o16).sum(-1, keepdim=True)), dt)
    p16 = round_to(p, dt)
    return round_to(scale * (ds16 @ k), dt), round_to(scale * (ds16.transpose(-1, -2) @ q), dt), round_to(p16.transpose(-1, -2) @ dout, dt)
