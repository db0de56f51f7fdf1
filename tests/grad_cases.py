"""Shared by tests/test_grad_sensitivity.py (CPU: every case can see its bug class, every case is kink-free) and
tests/test_gpu_grad_fp64.py (GPU: every parameter gradient of the fused backward against the fp64 oracle, per slice).

The older whole-model gradient checks compare against the fp32 oracle at rel 2e-3 of a tensor's largest gradient; a backward
chain that drops one 16-row tile, a cluster member's hidden chunk or one use of a shared block stays inside that.  A case here:

  * geometry      batch sizes picked by a restatement of the cluster geometry of the latent chains (chain.hip
                  launch_latent_chain, bchain.hip launch_latent_bchain): C = 4 / 2 / no cluster, idle members of a rounded grid;
  * slices        the error is measured per parameter tensor AND per slice -- a unit of the kernels' geometry (a head of to_q /
                  to_kv / to_out, a 16-row tile of the latents, a 128-unit hidden chunk of a feed-forward block) -- each slice
                  against its own fp64 maximum, so a slice that is small next to its tensor is still held;
  * kink repair   LeakyReLU (every to_out) and the SELU gate have derivative jumps at 0: an fp32 pre-activation within rounding of
                  0 may take either side, which moves a gradient row by O(1) however correct the kernel is.  Each case nudges the
                  bias of every column with a pre-activation closer to 0 than DELTA_FACTOR x the fp32 oracle's measured deviation
                  of that tensor, in execution order, until a whole fp64 forward finds none (``census`` re-checks it).  The
                  nudged set follows the host's fp32 / fp64 rounding (BLAS kernels, thread count), so it may differ between
                  hosts; the census is what every case must pass;
  * upstream      the gradient of the logits weights the first and the last sample up (EDGE_WEIGHT), so that their first / last
                  tiles -- where a chain's tile loop starts and ends -- carry a visible share of every shared weight's gradient;
  * mutations     the oracle's ``tap`` turns a case into what a backward with each bug class computes (``mutation_tap``).

The yardstick is tests/long_context_cases.py's (K, FLOOR["grad"], CEIL["grad"], SENSITIVITY), unchanged.
"""
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

import long_context_cases as LC
from oracle import healnet_cpu as O
from oracle import train_cpu as T

CR = 16                      # rows of a chain's row tile
CUS = 256                    # compute units of an MI355X
CHAIN_XCHG_FLAGS = 2048 + 1  # common.h
HIDDEN_CHUNK = 128           # hidden units of one cluster member's share at C = 4 (512 / 4)
DELTA_FACTOR = 50            # census: every kink input stays this many times the fp32 oracle's deviation away from 0
REPAIR_FACTOR = 100          # the repair clears twice that, so that the census holds with room after the nudges
CLEARANCE = 1.2              # a nudged column clears 1.2 x REPAIR_FACTOR x the deviation
ZERO_SLICE = 1e-6            # a slice whose fp64 maximum is below this fraction of its tensor's is zero in exact arithmetic
EDGE_WEIGHT = 4.0


# ---- restatement of the cluster geometry (chain.hip launch_latent_chain ~l.781-801, bchain.hip launch_latent_bchain ~l.584-600)
def _cdiv(a, b):
    return -(-a // b)


def geometry(b, l_c, backward=True, cus=CUS):
    """(tiles, gtiles, C) of a latent chain over b * l_c rows: C workgroups share a row tile; C = 1 is the per-tile grid."""
    tiles = _cdiv(b * l_c, CR)
    gtiles = _cdiv(tiles, 8) * 8
    C = 1
    if gtiles <= 128:
        c = 4 if gtiles <= 64 else 2
        fits = gtiles * c <= cus if backward else (gtiles * c <= 2 * cus and gtiles * c <= CHAIN_XCHG_FLAGS - 1)
        C = c if fits else 1
    return tiles, gtiles, C


def sweep_batches(l_c, bmax=64):
    """Both ends of every cluster regime (C = 4, 2, none) plus one batch inside the first: at l_c = 128, 1 / 3 / 8 / 9 / 16 / 17."""
    regimes: Dict[int, List[int]] = {}
    for b in range(1, bmax + 1):
        regimes.setdefault(geometry(b, l_c)[2], []).append(b)
    out = {regimes[4][0], min(regimes[4][0] + 2, regimes[4][-1]), regimes[4][-1], regimes[2][0], regimes[2][-1], regimes[1][0]}
    return sorted(out)


def idle_batches(l_c, bmax=64):
    """Per cluster regime the smallest batch whose last 8-tile group holds one or two real tiles (most idle workgroups): at
    l_c = 48, 3 / 22 / 43 (9 -> 16, 66 -> 72, 129 -> 136 tiles)."""
    out = {}
    for b in range(1, bmax + 1):
        tiles, _, C = geometry(b, l_c)
        if C not in out and tiles % 8 in (1, 2):
            out[C] = b
    return sorted(out.values())


def one_tile_batches(l_c):
    """The batches whose grid is one 8-tile group: the first (one tile) and the middle one (at l_c = 16: 1 and 5 tiles)."""
    bs = [b for b in range(1, 64) if geometry(b, l_c)[1] == 8]
    return [bs[0], bs[len(bs) // 2]]


# ---- models
SWEEP = dict(n_modalities=2, channel_dims=[300, 64], num_spatial_axes=[1, 1], out_dims=4, depth=2)
SWEEP_SHAPES = [(1, 300), (40, 64)]
SHARED = dict(n_modalities=3, channel_dims=[300, 64, 32], num_spatial_axes=[1, 1, 1], out_dims=4, depth=3, l_c=32,
              weight_tie_layers=True)
SHARED_SHAPES = [(1, 300), (40, 64), (24, 32)]
MISSING = dict(n_modalities=3, channel_dims=[50, 3, 64], num_spatial_axes=[1, 2, 1], out_dims=3, depth=2, l_c=32)
MISSING_SHAPES = [(1, 50), None, (90, 64)]
MASKED = dict(n_modalities=2, channel_dims=[30, 48], num_spatial_axes=[1, 1], out_dims=3, depth=2, l_c=32, x_heads=2, cross_dim_head=64)
MASKED_SHAPES = [(60, 30), (60, 48)]
STAGED_COMMON = dict(n_modalities=2, channel_dims=[200, 48], num_spatial_axes=[1, 1], out_dims=4, x_heads=1, l_heads=8,
                     self_per_cross_attn=0, num_freq_bands=2, max_freq=2.0)
STAGED = {   # the reference's tuned TCGA shapes (tests/test_gpu_staged.py TUNED) with both dropouts
    "brca": dict(depth=2, l_c=17, l_d=126, cross_dim_head=63, latent_dim_head=20, attn_dropout=0.4553, ff_dropout=0.3647),
    "kirp": dict(depth=5, l_c=17, l_d=62, cross_dim_head=27, latent_dim_head=113, attn_dropout=0.3179, ff_dropout=0.0474),
}
STAGED_SHAPES = [(1, 200), (70, 48)]
CFG4 = dict(LC.CFG4)
CFG4_SHAPES = [(1, 2000), (LC.BAG_ROWS, 768)]


def full_kw(kw):
    """The keywords with FusionConfig's defaults filled in (l_c, l_d, heads ... are read by the geometry and the slices)."""
    cfg = O.FusionConfig(**kw)
    return {k: getattr(cfg, k) for k in cfg.__dataclass_fields__}


@functools.lru_cache(maxsize=None)
def _alias_groups(kw_items):
    """canonical key -> every state_dict key of the same tensor, in the model's parameter order (weight tying)."""
    import healnet_amd as hn
    torch.manual_seed(0)
    model = hn.HealNet(**dict(kw_items))
    by_ptr: Dict[int, List[str]] = {}
    for k, v in model.state_dict().items():
        by_ptr.setdefault(v.data_ptr(), []).append(k)
    return {ks[0]: ks for ks in by_ptr.values()}


def alias_groups(kw):
    if not kw.get("weight_tie_layers"):
        return {k: [k] for k in O.state_dict_shapes(O.FusionConfig(**kw))}
    return _alias_groups(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))


@dataclass
class GradCase:
    name: str
    kw: dict
    b: int
    sd: Dict[str, torch.Tensor]                 # fp32 (kink-repaired), every key, aliases holding equal values
    ins: List[Optional[torch.Tensor]]           # fp64 holding fp32 values
    dl: Optional[torch.Tensor] = None           # (b, out_dims) upstream gradient of the logits, or
    surv: Optional[tuple] = None                # (y, c): the survival NLL of oracle/train_cpu.surv_nll
    mask: Optional[torch.Tensor] = None
    drop: Optional[Dict[int, torch.Tensor]] = None
    nudged: int = 0                             # bias columns the kink repair moved
    delta: Dict[tuple, float] = field(default_factory=dict)

    def cfg(self):
        return O.FusionConfig(**self.kw)

    def aliases(self):
        return alias_groups(self.kw)

    def present(self):
        return [t is not None for t in self.ins]


def _seeded_sd(kw, seed):
    sd = LC._state_dict(kw, seed, [])
    for ks in alias_groups(kw).values():
        for k in ks[1:]:
            sd[k] = sd[ks[0]].clone()
    return sd


def _inputs(shapes, b, seed):
    g = torch.Generator().manual_seed(seed)
    return [None if s is None else torch.rand(b, *s, generator=g).double() for s in shapes]


def _dl(b, out_dims):
    """A fixed upstream gradient, different per sample and logit; the first and last samples weighted EDGE_WEIGHT x."""
    idx = torch.arange(b * out_dims, dtype=torch.float64).reshape(b, out_dims)
    dl = torch.sin(0.7 * idx + 0.3) + 0.25
    w = torch.ones(b, 1, dtype=torch.float64)
    w[0] = w[-1] = EDGE_WEIGHT
    return dl * w


# ---- execution schedule (restates fusion_forward's order: per layer, per modality [cross, cross ff] if present, [self, self ff])
def schedule(cfg, present):
    out = []
    M = cfg.n_modalities
    for layer in range(cfg.depth):
        for m in range(M):
            if present[m]:
                out.append((f"layers.{layer}.{2 * m}.", "attn", m))
                out.append((f"layers.{layer}.{2 * m + 1}.", "ff", m))
            if cfg.self_per_cross_attn > 0:
                out.append((f"layers.{layer}.{2 * M}.0.", "attn", -1))
                out.append((f"layers.{layer}.{2 * M}.1.", "ff", -1))
    return out


def _bias_key(sched, step, site):
    pfx, kind, _ = sched[step]
    assert (site == "attn_pre") == (kind == "attn"), (step, site, kind)
    return pfx + ("fn.to_out.0.bias" if kind == "attn" else "fn.net.0.bias")


def _forward(case_like, sd, dtype, tap=None, device="cpu"):
    kw, ins, mask, drop = case_like
    xs = [None if t is None else t.to(device=device, dtype=dtype) for t in ins]
    d = None if drop is None else {k: v.to(device=device, dtype=dtype) for k, v in drop.items()}
    with torch.device(device):
        return O.fusion_forward(sd, O.FusionConfig(**kw), xs, mask=None if mask is None else mask.to(device), drop=d, tap=tap)


def kink_inputs(case_like, sd, dtype):
    """{(step, site): tensor} of every LeakyReLU and gate input of one forward in the given precision, and the logits."""
    rec = {}

    def tap(step, site, t):
        if site in ("attn_pre", "gate"):
            rec[(step, site)] = t.detach().double()
        return t

    with torch.no_grad():
        y = _forward(case_like, {k: v.to(dtype) for k, v in sd.items()}, dtype, tap)
    return rec, y


def _deviation(case_like, sd):
    r64, _ = kink_inputs(case_like, sd, torch.float64)
    r32, _ = kink_inputs(case_like, sd, torch.float32)
    return {k: float((r32[k] - r64[k]).abs().max()) for k in r64}, r64


def _column_shift(v, w):
    """The smallest |t| with min |v + t| >= w over the values v of one column."""
    c, _ = torch.sort(-v)
    lo, hi = c - w, c + w
    # merge the forbidden intervals (lo_i, hi_i) and return the nearer edge of the one holding 0
    start, end = float(lo[0]), float(hi[0])
    for a, e in zip(lo[1:].tolist(), hi[1:].tolist()):
        if a <= end:
            end = max(end, e)
            continue
        if start < 0 < end:
            break
        start, end = a, e
    if not (start < 0 < end):
        return 0.0
    return start if -start < end else end


def repair(case_like, sd, max_passes=24):
    """Nudges bias columns (to_out.0.bias, the gate half of net.0.bias) in place until no kink input of the fp64 forward lies within
    REPAIR_FACTOR x the fp32 oracle's deviation of that tensor.  -> (number of nudged columns, {(step, site): delta})."""
    dev, _ = _deviation(case_like, sd)
    delta = {k: REPAIR_FACTOR * v for k, v in dev.items()}
    cfg = O.FusionConfig(**case_like[0])
    sched = schedule(cfg, [t is not None for t in case_like[1]])
    groups = alias_groups(case_like[0])
    alias_of = {k: ks for ks in groups.values() for k in ks}
    nudged = 0
    for npass in range(max_passes):
        sd64 = {k: v.double() for k, v in sd.items()}
        for ks in groups.values():          # tied keys share one tensor, so a nudge reaches every alias
            for k in ks[1:]:
                sd64[k] = sd64[ks[0]]
        seen: Dict[str, torch.Tensor] = {}  # canonical bias key -> earlier values of its columns in this pass
        moved, closest = [0], [float("inf")]

        def tap(step, site, t):
            if site not in ("attn_pre", "gate"):
                return t
            key = alias_of[_bias_key(sched, step, site)][0]
            n = t.shape[-1]
            off = 0 if site == "attn_pre" else sd64[key].numel() - n
            vals = t.detach().reshape(-1, n)
            allv = vals if key not in seen else torch.cat([seen[key], vals])
            w = delta[(step, site)]
            near = (allv.abs() < w).any(0).nonzero().flatten().tolist()
            shift = torch.zeros(n, dtype=t.dtype)
            for j in near:
                want = _column_shift(allv[:, j], CLEARANCE * w)
                bias = sd64[key][off + j]
                new = float(torch.tensor(float(bias) + want).float())     # the case's weights are fp32
                shift[j] = new - float(bias)
                sd64[key][off + j] = new
                moved[0] += 1
            seen[key] = allv + shift
            closest[0] = min(closest[0], float(vals.abs().min()) / w)
            return t + shift if near else t

        with torch.no_grad():
            _forward(case_like, sd64, torch.float64, tap)
        for k in sd:
            sd[k] = sd64[alias_of.get(k, [k])[0]].float().clone()
        nudged += moved[0]
        # done when a whole forward finds nothing to nudge, or nothing within the census distance (DELTA_FACTOR) before its
        # nudges: a block used several times per forward (the latent self block, tied layers) is re-run after a nudge of a later
        # use, which can bring back a column near the REPAIR_FACTOR edge pass after pass
        if moved[0] == 0 or closest[0] >= DELTA_FACTOR / REPAIR_FACTOR:
            return nudged, delta
    raise AssertionError(f"kink repair did not converge in {max_passes} passes")


def census(case):
    """-> (worst margin, worst logit-clamp ratio): min over kink inputs of |pre| / (DELTA_FACTOR x fp32 deviation) -- >= 1 is
    kink-free -- and, with the survival loss, min over the clamped terms of value / eps."""
    cl = (case.kw, case.ins, case.mask, case.drop)
    dev, r64 = _deviation(cl, case.sd)
    worst = min(float(r64[k].abs().min()) / max(DELTA_FACTOR * dev[k], 1e-300) for k in r64)
    clamp = float("inf")
    if case.surv is not None:
        y, c = case.surv
        with torch.no_grad():
            logits = _forward(cl, {k: v.double() for k, v in case.sd.items()}, torch.float64)
        _, _, hz, S = T.surv_nll(logits, y, c)
        Sp = torch.cat([torch.ones_like(S[:, :1]), S], 1)
        Y = y.view(-1, 1)
        terms = torch.cat([torch.gather(Sp, 1, Y), torch.gather(hz, 1, Y), torch.gather(Sp, 1, Y + 1)])
        clamp = float(terms.min()) / 1e-7
    return worst, clamp


def _finish(name, kw, b, sd, ins, dl=None, surv=None, mask=None, drop=None):
    kw = full_kw(kw)
    ins = LC.fp32_inputs(ins)
    nudged, delta = repair((kw, ins, mask, drop), sd)
    return GradCase(name, kw, b, sd, ins, dl=dl, surv=surv, mask=mask, drop=drop, nudged=nudged, delta=delta)


@functools.lru_cache(maxsize=None)
def sweep_case(b, l_c=128, snn=True):
    kw = dict(SWEEP, l_c=l_c, snn=snn)
    return _finish(f"sweep_lc{l_c}_b{b}" + ("" if snn else "_gelu"), kw, b, _seeded_sd(kw, 31), _inputs(SWEEP_SHAPES, b, 32),
                   dl=_dl(b, kw["out_dims"]))


@functools.lru_cache(maxsize=None)
def shared_case(b=4):
    return _finish("shared_tied", SHARED, b, _seeded_sd(SHARED, 41), _inputs(SHARED_SHAPES, b, 42), dl=_dl(b, SHARED["out_dims"]))


@functools.lru_cache(maxsize=None)
def missing_case(b=8):
    return _finish("missing", MISSING, b, _seeded_sd(MISSING, 51), _inputs(MISSING_SHAPES, b, 52), dl=_dl(b, MISSING["out_dims"]))


def key_mask(b, n, seed=63):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(b, n, generator=g) > 0.3
    mask[:, 0] = True
    return mask


@functools.lru_cache(maxsize=None)
def masked_case(b=4):
    return _finish("masked", MASKED, b, _seeded_sd(MASKED, 61), _inputs(MASKED_SHAPES, b, 62), dl=_dl(b, MASKED["out_dims"]),
                   mask=key_mask(b, MASKED_SHAPES[0][0]))


def staged_kw(name):
    return dict(STAGED_COMMON, **STAGED[name])


def drop_shapes(kw, b, present):
    """{step: (shape, p)} of the dropout multipliers fusion_forward takes (numbered like test_gpu_dropout._oracle_masks)."""
    cfg = O.FusionConfig(**kw)
    shapes = [s for s in STAGED_SHAPES]
    n_tok = [1 if s is None else int(torch.tensor(s[:-1]).prod()) for s in shapes]
    out, k = {}, 0
    for pfx, kind, m in schedule(cfg, present):
        if kind == "attn" and cfg.attn_dropout > 0:
            h = cfg.x_heads if m >= 0 else cfg.l_heads
            out[k] = ((b * h, cfg.l_c, n_tok[m] if m >= 0 else cfg.l_c), cfg.attn_dropout)
        if kind == "ff" and cfg.ff_dropout > 0:
            out[k] = ((b, cfg.l_c, cfg.l_d), cfg.ff_dropout)
        k += 1
    return out


def random_drop(kw, b, seed=71):
    """Bernoulli multipliers of the case's shapes (the CPU check's stand-in for the build's exported masks)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, (shape, p) in drop_shapes(kw, b, [True, True]).items():
        out[k] = (torch.rand(shape, generator=g) >= p).double() / (1 - p)
    return out


def staged_case(name, drop, b=3):
    """The tuned TCGA shape under the given dropout multipliers (the GPU test passes the build's exported masks): not cached."""
    kw = staged_kw(name)
    return _finish(f"staged_{name}", kw, b, _seeded_sd(kw, 81), _inputs(STAGED_SHAPES, b, 82), dl=_dl(b, kw["out_dims"]),
                   drop={k: v.double() for k, v in drop.items()})


@functools.lru_cache(maxsize=None)
def cfg4_case(b=2):
    """The bench's training-step shape: omic 1 x 2000 + bag 4096 x 768, depth 3, survival NLL."""
    g = torch.Generator().manual_seed(92)
    y = torch.randint(0, CFG4["out_dims"], (b,), generator=g)
    c = torch.tensor([i % 2 for i in range(b)])
    return _finish(f"cfg4_b{b}", CFG4, b, _seeded_sd(CFG4, 91), _inputs(CFG4_SHAPES, b, 93), surv=(y, c))


# ---- oracle gradients of every parameter
def oracle_grads(case, device="cpu", dtype=torch.float64, tap=None, drop=None):
    """d loss / d p for every canonical parameter key (tied aliases summed), by autograd through the oracle.  Loss: sum(logits * dl)
    or the survival NLL.  ``drop`` overrides the case's dropout multipliers (the mask-slip mutation)."""
    sd = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in case.sd.items()}
    y = _forward((case.kw, case.ins, case.mask, case.drop if drop is None else drop), sd, dtype, tap, device)
    if case.surv is not None:
        _, g, _, _ = T.surv_nll(y.detach(), case.surv[0].to(device), case.surv[1].to(device))
        (y * g).sum().backward()
    else:
        (y * case.dl.to(device=device, dtype=dtype)).sum().backward()
    out = {}
    for k, ks in case.aliases().items():
        out[k] = sum(sd[a].grad.detach() if sd[a].grad is not None else torch.zeros_like(sd[a]) for a in ks)
    return out


# ---- slices: units of the kernels' geometry
def slices(case, key, shape):
    """[(label, index)] of the slices of one parameter tensor (the whole tensor is always checked as well)."""
    kw = case.kw
    M = kw["n_modalities"]
    parts = key.split(".")
    out = []
    if key == "latents":
        for t in range(_cdiv(shape[0], CR)):
            out.append((f"tile{t}", (slice(t * CR, (t + 1) * CR),)))
        return out
    if parts[0] != "layers":
        return out
    cross = int(parts[2]) < 2 * M
    heads, e = (kw["x_heads"], kw["cross_dim_head"]) if cross else (kw["l_heads"], kw["latent_dim_head"])
    inner = heads * e
    leaf = ".".join(parts[-3:]) if "to_" in key else ".".join(parts[-2:])
    if leaf == "to_q.weight":
        out = [(f"h{h}", (slice(h * e, (h + 1) * e),)) for h in range(heads)]
    elif leaf == "to_kv.weight":
        out = [(f"K.h{h}", (slice(h * e, (h + 1) * e),)) for h in range(heads)]
        out += [(f"V.h{h}", (slice(inner + h * e, inner + (h + 1) * e),)) for h in range(heads)]
    elif key.endswith("to_out.0.weight"):
        out = [(f"h{h}", (slice(None), slice(h * e, (h + 1) * e))) for h in range(heads)]
    elif key.endswith("net.0.weight") or key.endswith("net.0.bias"):
        hid = shape[0] // 2
        for c in range(_cdiv(hid, HIDDEN_CHUNK)):
            lo, hi = c * HIDDEN_CHUNK, min(hid, (c + 1) * HIDDEN_CHUNK)
            out.append((f"value{c}", (slice(lo, hi),)))
            out.append((f"gate{c}", (slice(hid + lo, hid + hi),)))
    elif key.endswith("net.2.weight"):
        hid = shape[1]
        out = [(f"hidden{c}", (slice(None), slice(c * HIDDEN_CHUNK, min(hid, (c + 1) * HIDDEN_CHUNK))))
               for c in range(_cdiv(hid, HIDDEN_CHUNK))]
    return out


def grad_scale(ref):
    """The largest fp64 gradient of the case: the absolute scale of tensors that are zero in exact arithmetic."""
    return max(float(v.abs().max()) for v in ref.values())


def slice_errors(case, key, got, ref, scale):
    """[(label, error, zero)] of the whole tensor and every slice: max |got - ref| over the slice / the slice's fp64 maximum, or,
    for a slice that is zero in exact arithmetic (zero = True), / its tensor's maximum -- / ``scale`` for a whole tensor that is
    (the query side of a one-token block)."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    tmax = float(ref.abs().max())
    if tmax < ZERO_SLICE * scale:
        return [("all", float((got - ref).abs().max()) / scale, True)]
    out = [("all", float((got - ref).abs().max()) / tmax, False)]
    for label, idx in slices(case, key, tuple(ref.shape)):
        g, r = got[idx], ref[idx]
        smax = float(r.abs().max())
        zero = smax < ZERO_SLICE * tmax
        out.append((label, float((g - r).abs().max()) / max(tmax if zero else smax, 1e-300), zero))
    return out


def max_slice_shift(case, got, ref):
    """The largest slice error of one gradient set against another (mutation shift), with its location."""
    best = (0.0, "")
    scale = grad_scale(ref)
    for k in ref:
        for label, e, zero in slice_errors(case, k, got[k], ref[k], scale):
            if not zero and e > best[0]:
                best = (e, f"{k}[{label}]")
    return best


# ---- mutations through the oracle's tap
class _SampleSlip(torch.autograd.Function):
    """Identity forward; backward hands sample s's gradient to sample s + 1."""

    @staticmethod
    def forward(ctx, t, s):
        ctx.s = s
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[ctx.s + 1] = g[ctx.s]
        return g, None


def _grad_mask(t, keep):
    """t in the forward (exactly: keep is 0 / 1); the gradient only where keep is 1."""
    return t * keep + (t * (1 - keep)).detach()


def tile_rows(case, tile):
    """(sample, row) pairs of the flat row tile of a chain over b * l_c rows."""
    L = case.kw["l_c"]
    return [divmod(r, L) for r in range(tile * CR, min((tile + 1) * CR, case.b * L))]


def latent_ff_step(case, layer=0):
    """Execution index of the last feed-forward block of a layer (the latent self block's, when there is one)."""
    sched = schedule(case.cfg(), case.present())
    return max(i for i, (pfx, kind, _) in enumerate(sched) if kind == "ff" and pfx.startswith(f"layers.{layer}."))


def latent_attn_step(case, layer=0, use=0):
    """Execution index of a use of the latent self-attention block of a layer (or of the first cross block without one)."""
    sched = schedule(case.cfg(), case.present())
    uses = [i for i, (pfx, kind, m) in enumerate(sched) if kind == "attn" and m < 0 and pfx.startswith(f"layers.{layer}.")]
    return uses[use]


def mutation_tap(case, kind, **a):
    """A tap that makes the oracle's backward commit one bug class:
      lost_tile    tile a["tile"]'s backward through block a["step"] is missing (its rows' gradient stops at the block's branch);
      lost_member  hidden units a["lo"]:a["hi"] of tile a["tile"] are missing from block a["step"]'s feed-forward backward (the
                   gradient of z is cut there; a real lost member would also lose its net.2 columns, a larger shift);
      sample_slip  block a["step"] takes sample a["s"]'s upstream gradient for sample a["s"] + 1;
      lost_use     one use (block a["step"]) of a shared block is not accumulated."""
    step = a["step"]

    def tap(k, site, t):
        if k != step:
            return t
        if kind in ("lost_tile", "lost_member") and site == ("out" if kind == "lost_tile" else "z"):
            keep = torch.ones_like(t)
            cols = slice(None) if kind == "lost_tile" else slice(a["lo"], a["hi"])
            for s, r in tile_rows(case, a["tile"]):
                keep[s, r, cols] = 0
            return _grad_mask(t, keep)
        if kind == "sample_slip" and site == "out":
            return _SampleSlip.apply(t, a["s"])
        if kind == "lost_use" and site == "out":
            return t.detach()
        return t

    return tap


def shift_mask(drop, step):
    """mask slip: block step's dropout multipliers moved by one latent row."""
    out = dict(drop)
    out[step] = torch.roll(drop[step], 1, dims=1)
    return out
