"""Shared by tests/test_long_context_sensitivity.py (CPU: proves every case can see its bug class) and tests/test_gpu_long_context.py
(GPU: the HIP attention cores at production context lengths against the fp64 oracle).

The whole-model checks at full size compare against an fp32 oracle on torch.rand inputs, where attention over 50 k tokens is nearly
uniform and no single token matters.  A case here is built so that single tokens DO matter:

  * sharpened queries   the to_q weights of the long-context cross blocks are scaled (SHARPEN), so each latent row concentrates on a
                        few tokens;
  * needles             distinctive tokens at 0, 15, 16, N - 1, the last 16-token step and both sides of every token-split boundary
                        of the forward and backward plans (a restatement of attn_core_geometry, healnet_amd/csrc/attention.hip), plus
                        a few positions that differ per sample, so a per-sample stride slip shows;
  * masked needles      (bag cases with a key mask) a huge needle on a masked row: the reference ignores it, a leak is O(1);
  * mutations           copies of the inputs with one region corrupted -- what the core would compute under each bug class.

If the kernels' plan changes, the needles only lose their boundary property; the cases stay valid.
"""
from dataclasses import dataclass
from typing import Dict

import torch

from oracle import healnet_cpu as O

SHARPEN = 32.0
L_C = 128

# ---- the yardstick (tests/test_gpu_x6.py's): a HIP result's error against fp64 must be <= K x the fp32 oracle's error on the same
# inputs, or under FLOOR, whichever is larger -- and that bound itself must stay under CEIL, the figure the CPU self-check proves
# every mutation exceeds by SENSITIVITY x.
K = 8
SENSITIVITY = 20
FLOOR = {"fp32": 2e-6, "probs": 2e-6, "grad": 2e-5}
CEIL = {"fp32": 2e-5, "probs": 1e-3, "grad": 5e-4, "bf16x3": 1e-3, "bf16": 2e-2}

CFG2 = dict(n_modalities=2, channel_dims=[2000, 3], num_spatial_axes=[1, 2], out_dims=4)
CFG3 = dict(n_modalities=3, channel_dims=[2000, 3, 3], num_spatial_axes=[1, 2, 3], out_dims=4)
CFG4 = dict(n_modalities=2, channel_dims=[2000, 768], num_spatial_axes=[1, 1], out_dims=4)
BAG1 = dict(n_modalities=1, channel_dims=[768], num_spatial_axes=[1], out_dims=4)      # one bag: the mask= path applies to it alone

IMG = (224, 224)
BAG_ROWS = 4096
VOL_FRAMES = 4


# ---- restatement of the token-split plan (healnet_amd/csrc/attention.hip: attn_core_geometry, attn_core_nq_small_batch;
# api_blocks.hip: plan_attn, context_pitch) -- default knobs, fp32 core
CHAIN_MERGE_MAX_SPLITS = 48


def _cdiv(a, b):
    return -(-a // b)


def _pad_head_dim(dh):
    return 16 if dh <= 16 else 32 if dh <= 32 else 64 if dh <= 64 else 128


def context_pitch(D, dim_head=64):
    dp = 16 if D <= 15 else (32 if D <= 31 else 0)
    if dp and dp <= _pad_head_dim(dim_head):
        return dp
    return _cdiv(D, 4) * 4


def _nq_small_batch(dp, b, h, Lp):
    if dp != 16:
        return 0
    tiles = Lp // 16
    for c in (4, 2, 1):
        if b * h * _cdiv(tiles, c) >= 128:
            return c
    return 1 if b * h * tiles * CHAIN_MERGE_MAX_SPLITS >= 512 else 0


def core_geometry(b, h, Lp, N, dp, waves_per_simd=0, nq=0):
    """(nsplit, chunk) of attn_core_geometry."""
    dt = dp // 16
    nq_eff = nq if nq > 0 else (4 if dt == 1 else 2 if dt in (2, 4) else 1)
    ngroups = _cdiv(Lp // 16, nq_eff)
    tw = 1024 * waves_per_simd if waves_per_simd > 0 else 4096
    want = tw // (b * h * ngroups)
    if nq > 0:
        want = min(want, CHAIN_MERGE_MAX_SPLITS)
    want = max(1, min(want, max(1, N // 128)))
    c = _cdiv(_cdiv(N, want), 16) * 16
    return _cdiv(N, c), c


def split_plans(b, N, D, heads=8, dim_head=64, L=L_C):
    """{"fwd": chunk, "bwd": chunk} of plan_attn for a cross block over N tokens of width D."""
    ld = context_pitch(D, dim_head)
    dhp = _pad_head_dim(dim_head)
    rank_d = ld in (16, 32) and D <= ld <= dhp
    dp = ld if rank_d else dhp
    Lp = _cdiv(L, 16) * 16
    nq = _nq_small_batch(dp, b, heads, Lp) if rank_d else 0
    _, fwd = core_geometry(b, heads, Lp, N, dp, 0, nq)
    _, bwd = core_geometry(b, heads, Lp, N, dp, 2 if (not rank_d and dp == 64 and N >= 256) else 3)
    return {"fwd": fwd, "bwd": bwd}


def split_edges(N, chunk):
    """First token of every split after the first."""
    return list(range(chunk, N, chunk))


# ---- needles
def needle_positions(N, chunks, sample):
    """Sorted token positions of one sample's needles: the fixed edges of every plan plus three sample-dependent positions."""
    pos = {0, 15, 16, N - 1, N - 2, N - 9, N - 16 if N >= 16 else 0}
    for c in chunks:
        for e in split_edges(N, c):
            pos.update((e - 1, e, e - 16, e + 15))
    for k in range(3):
        pos.add((7919 * (sample + 1) * (k + 3) + 101 * k) % N)
    return sorted(p for p in pos if 0 <= p < N)


def range_end_positions(N, chunk):
    """The tokens of the last 16-token step of every split (the last split's may be partial)."""
    out = []
    starts = [0] + split_edges(N, chunk)
    for s in starts:
        e = min(s + chunk, N)
        last = s + ((e - s - 1) // 16) * 16
        out.extend(range(last, e))
    return out


def _needle_rows(seed, count, width):
    """count needle rows (width channels): a few large channels each, different per row and seed -- after the context LayerNorm
    each points in a direction no smooth background row has."""
    g = torch.Generator().manual_seed(seed)
    v = torch.zeros(count, width, dtype=torch.float64)
    hot = min(3, width)
    for j in range(count):
        idx = torch.randperm(width, generator=g)[:hot]
        v[j, idx] = (torch.rand(hot, generator=g, dtype=torch.float64) * 4 + 4) * (torch.randint(0, 2, (hot,), generator=g) * 2 - 1)
    return v


def _background(shape, salt):
    """Smooth, low-contrast rows: every background token looks much like its neighbours."""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, dtype=torch.float64)
    return (0.5 + 0.1 * torch.sin(0.013 * idx + salt) * torch.cos(0.0007 * idx + 0.3 * salt)).reshape(shape)


def _put(flat_rows, sample, positions, width, salt=0):
    flat_rows[torch.tensor(positions)] += _needle_rows(1000 * sample + 17 + 37 * salt, len(positions), width)


@dataclass
class Case:
    name: str
    kw: dict                                   # HealNet / FusionConfig keywords
    sd: Dict[str, torch.Tensor]                # fp32 state dict (reference key layout)
    long_m: int                                # modality index of the long context
    N: int
    plans: Dict[int, Dict[str, int]]           # batch -> {"fwd", "bwd"} chunks used for the needles

    def cfg(self):
        return O.FusionConfig(**self.kw)

    def sd64(self):
        return {k: v.double() for k, v in self.sd.items()}


def _state_dict(kw, seed, sharpen_modalities):
    """Seeded weights with Linear-like scales; the to_q of every long-context cross block scaled by SHARPEN."""
    cfg = O.FusionConfig(**kw)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in O.state_dict_shapes(cfg).items():
        leaf = k.split(".")[-1]
        if k == "latents":
            t = torch.randn(shape, generator=g)
        elif (".norm" in k or k.startswith("to_logits.1")) and leaf == "weight":
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif leaf == "bias":
            t = 0.05 * torch.randn(shape, generator=g)
        else:
            bound = shape[-1] ** -0.5
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        sd[k] = t.float()
    for layer in range(cfg.depth):
        for m in sharpen_modalities:
            key = f"layers.{layer}.{2 * m}.fn.to_q.weight"
            sd[key] = sd[key] * SHARPEN
    return sd


def make_case(name, kw, long_m, N, batches, seed=11):
    kw = dict(kw)
    D = O.FusionConfig(**kw).context_dim(long_m)
    plans = {b: split_plans(b, N, D) for b in batches}
    return Case(name, kw, _state_dict(kw, seed, [long_m]), long_m, N, plans)


def image_case(depth=1, batches=(1, 2, 8, 32)):
    return make_case(f"cfg2_d{depth}", dict(CFG2, depth=depth), 1, IMG[0] * IMG[1], batches)


def volume_case():
    return make_case("cfg3_vol4", dict(CFG3, depth=1), 2, VOL_FRAMES * IMG[0] * IMG[1], (2,))


def bag_case(batches=(1, 2, 8)):
    return make_case("cfg4", dict(CFG4, depth=1), 1, BAG_ROWS, batches)


def masked_bag_case():
    return make_case("bag_masked", dict(BAG1, depth=1), 0, BAG_ROWS, (2,))


def _all_chunks(case):
    out = set()
    for p in case.plans.values():
        out.update(p.values())
    return sorted(out)


def long_input(case, samples):
    """(len(samples), *spatial, C) fp64 long-context input of the given sample indices (a row subset of a larger batch is the same
    rows as in the full batch)."""
    C = case.kw["channel_dims"][case.long_m]
    chunks = _all_chunks(case)
    rows = []
    for s in samples:
        x = _background((case.N, C), salt=case.long_m + 0.01 * s)
        _put(x, s, needle_positions(case.N, chunks, s), C)
        rows.append(x)
    x = torch.stack(rows)
    axes = case.kw["num_spatial_axes"][case.long_m]
    if axes == 1:
        return x
    if axes == 2:
        return x.reshape(len(samples), *IMG, C)
    return x.reshape(len(samples), case.N // (IMG[0] * IMG[1]), *IMG, C)


def inputs(case, samples):
    """All modalities (fp64) for the sample indices; the short modalities are smooth per-sample rows."""
    out = []
    for m in range(case.kw["n_modalities"]):
        if m == case.long_m:
            out.append(long_input(case, samples))
            continue
        C = case.kw["channel_dims"][m]
        axes = case.kw["num_spatial_axes"][m]
        if axes == 1 and C == 2000:
            rows = [_background((1, C), salt=m + 0.37 * s) for s in samples]
        else:      # a short image next to a volume: 224 x 224 background with needles at its own split edges
            n = IMG[0] * IMG[1]
            chunks = sorted(set(split_plans(b, n, O.FusionConfig(**case.kw).context_dim(m))["fwd"] for b in case.plans))
            rows = []
            for s in samples:
                x = _background((n, C), salt=m + 0.01 * s)
                _put(x, s, needle_positions(n, chunks, s), C, salt=1)
                rows.append(x.reshape(*IMG, C))
        out.append(torch.stack(rows))
    return out


def bag_mask(case, samples):
    """(len(samples), N) key mask: the last 300 + 50 s rows of each sample are padding; one padding row holds a huge needle."""
    N = case.N
    mask = torch.ones(len(samples), N, dtype=torch.bool)
    for i, s in enumerate(samples):
        mask[i, N - 300 - 50 * s:] = False
    return mask


def masked_needle_row(case, sample):
    return case.N - 100 - 7 * sample


def masked_inputs(case, samples):
    """Inputs of the masked-bag case: padding rows zero (as a loader pads), one of them a huge needle the mask hides."""
    ins = inputs(case, samples)
    mask = bag_mask(case, samples)
    x = ins[case.long_m]
    for i, s in enumerate(samples):
        x[i][~mask[i]] = 0.0
        x[i, masked_needle_row(case, s)] = 1e3 * _needle_rows(99 + s, 1, x.shape[-1])[0]
    return ins, mask


# ---- mutations: what a core with each bug class would have computed
def mutate(case, ins, samples, kind, b, mask=None):
    """A copy of (ins, mask) with one region corrupted, for the batch size b whose plan the needles target.
      range_ends    the last 16-token step of every forward split of the LAST sample replaced by background (a skipped end tile);
      bwd_range_ends  the same for the backward plan;
      range_starts  the first 16-token step of every split of the last sample (a skipped first tile / a shifted range);
      stride        the last sample's long context replaced by sample 0's (a per-sample stride slip);
      unmask        the masked needle made visible (a masked token leaking into the softmax)."""
    ins = [t.clone() for t in ins]
    mask = None if mask is None else mask.clone()
    x = ins[case.long_m]
    C = x.shape[-1]
    i = len(samples) - 1
    flat = x[i].reshape(case.N, C)
    bg = _background((case.N, C), salt=case.long_m + 0.01 * samples[i])
    if kind in ("range_ends", "bwd_range_ends"):
        chunk = case.plans[b]["fwd" if kind == "range_ends" else "bwd"]
        pos = torch.tensor(range_end_positions(case.N, chunk))
        flat[pos] = bg[pos]
    elif kind == "range_starts":
        chunk = case.plans[b]["fwd"]
        pos = torch.tensor([s + k for s in [0] + split_edges(case.N, chunk) for k in range(16) if s + k < case.N])
        flat[pos] = bg[pos]
    elif kind == "stride":
        x[i] = long_input(case, [samples[0]])[0]
    elif kind == "unmask":
        mask[i, masked_needle_row(case, samples[i])] = True
    else:
        raise ValueError(kind)
    return ins, mask


# ---- the error measure every test uses
def err(a, ref):
    """max |a - ref| / max |ref| (both promoted to fp64 on the CPU)."""
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def fp32_inputs(ins):
    """The inputs as the HIP path sees them: every reference runs on the fp32-rounded values."""
    return [None if t is None else t.float().double() for t in ins]


def long_block_keys(case):
    """Parameter names of the long-context cross-attention blocks."""
    return [k for k in case.sd if any(k.startswith(f"layers.{L}.{2 * case.long_m}.") for L in range(case.cfg().depth))]


def oracle_grads(case, ins, dl, mask=None, device="cpu", dtype=torch.float64):
    """Gradients of sum(logits * dl) w.r.t. the long-context cross blocks' parameters by autograd through the oracle."""
    keys = long_block_keys(case)
    sd = {k: v.to(device=device, dtype=dtype) for k, v in case.sd.items()}
    for k in keys:
        sd[k].requires_grad_(True)
    xs = [None if t is None else t.to(device=device, dtype=dtype) for t in ins]
    with torch.device(device):
        y = O.fusion_forward(sd, case.cfg(), xs, mask=None if mask is None else mask.to(device))
        (y * dl.to(device=device, dtype=dtype)).sum().backward()
    return {k: sd[k].grad.detach() for k in keys}


def oracle(case, ins, mask=None, return_embeddings=True, device="cpu", dtype=torch.float64, token_chunk=None):
    """The pinned oracle in the given precision on the given device (torch's factory default device is switched so that the
    oracle's own linspace grids land there too)."""
    sd = {k: v.to(device=device, dtype=dtype) for k, v in case.sd.items()}
    xs = [None if t is None else t.to(device=device, dtype=dtype) for t in ins]
    m = None if mask is None else mask.to(device)
    with torch.device(device), torch.no_grad():
        return O.fusion_forward(sd, case.cfg(), xs, mask=m, return_embeddings=return_embeddings, token_chunk=token_chunk)
