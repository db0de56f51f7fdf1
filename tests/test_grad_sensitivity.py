"""CPU self-check of tests/test_gpu_grad_fp64.py: in fp64 on the host, every bug class of a backward chain -- a lost 16-row tile, a
cluster member's lost hidden chunk, a sample slip, a use of a shared block that is not accumulated, a dropout mask shifted by one
row -- moves at least one checked gradient slice by SENSITIVITY x the GPU test's ceiling; every case is kink-free (census); the
cluster-geometry restatement gives the documented transitions; and the oracle's tap leaves the computation untouched."""
import pytest
import torch

import grad_cases as G
import long_context_cases as LC
from oracle import healnet_cpu as O

BOUND = LC.CEIL["grad"]


def _require(case, what, mutated, ref):
    shift, where = G.max_slice_shift(case, mutated, ref)
    print(f"{case.name} {what}: shift {shift:.3e} at {where} ({shift / BOUND:.0f} x the bound {BOUND:.0e})")
    assert shift >= LC.SENSITIVITY * BOUND, f"{case.name} {what}: shift {shift:.3e} < {LC.SENSITIVITY} x {BOUND:.0e}"


def _census(case):
    worst, clamp = G.census(case)
    print(f"{case.name}: {case.nudged} bias columns nudged, kink margin {worst:.2f} x {G.DELTA_FACTOR} x the fp32 deviation, "
          f"survival clamp margin {clamp:.1e}")
    assert worst >= 1.0, f"{case.name}: a kink input lies within {G.DELTA_FACTOR} x the fp32 oracle's deviation of 0"
    assert clamp >= 1e3, f"{case.name}: a survival-loss term is within 1e3 x eps of its clamp"


def test_geometry_transitions():
    """for <= 128 row tiles C = 4 / 2 workgroups share a tile (4 up to 64 tiles); the grid's member rows are a
    multiple of 8 tiles; beyond 128 tiles no cluster.  The sweeps hit both sides of every transition."""
    assert [G.geometry(b, 128)[2] for b in G.sweep_batches(128)] == [4, 4, 4, 2, 2, 1]
    assert [G.geometry(b, 128)[0] for b in G.sweep_batches(128)] == [8, 24, 64, 72, 128, 136]
    assert [G.geometry(b, 48)[:3] for b in G.idle_batches(48)] == [(9, 16, 4), (66, 72, 2), (129, 136, 1)]
    assert [G.geometry(b, 16)[:2] for b in G.one_tile_batches(16)] == [(1, 8), (5, 8)]
    for b in range(1, 40):
        for l_c in (16, 48, 128):
            tiles, gtiles, C = G.geometry(b, l_c)
            assert gtiles % 8 == 0 and 0 <= gtiles - tiles < 8
            assert C == (4 if gtiles <= 64 else 2 if gtiles <= 128 else 1)
            assert G.geometry(b, l_c, backward=False)[2] == C        # at 256 CUs both launches agree
    assert G.geometry(16, 128, cus=128)[2] == 1 and G.geometry(16, 128, backward=False, cus=128)[2] == 2


def test_oracle_tap_is_transparent():
    """fusion_forward with tap=None and with an identity tap: the same logits and gradients, bit for bit (dropout, a mask and a
    missing modality on the way)."""
    kw = dict(n_modalities=3, channel_dims=[20, 3, 12], num_spatial_axes=[1, 2, 1], out_dims=3, depth=2, l_c=16, l_d=32, x_heads=2,
              l_heads=2, cross_dim_head=16, latent_dim_head=16, attn_dropout=0.2, ff_dropout=0.1)
    cfg = O.FusionConfig(**kw)
    g = torch.Generator().manual_seed(5)
    sd0 = {k: torch.randn(s, generator=g) * 0.3 for k, s in O.state_dict_shapes(cfg).items()}
    b = 2
    ins = [torch.rand(b, 1, 20, generator=g), None, torch.rand(b, 7, 12, generator=g)]
    mask = torch.rand(b, 7, generator=g) > 0.3
    mask[:, 0] = True
    drop = {0: (torch.rand(b * 2, 16, 1, generator=g) > 0.2).float() / 0.8, 1: (torch.rand(b, 16, 32, generator=g) > 0.1).float() / 0.9}
    seen = []
    out = []
    for tap in (None, lambda k, site, t: (seen.append((k, site)), t)[1]):
        sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
        y = O.fusion_forward(sd, cfg, [ins[0], None, None], drop=drop, tap=tap)
        y2 = O.fusion_forward(sd, cfg, [None, None, ins[2]], mask=mask, tap=tap)
        (y.sum() + (y2 * torch.arange(3.0)).sum()).backward()
        out.append((y.detach(), y2.detach(), {k: v.grad for k, v in sd.items()}))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    for k in sd0:
        a, c = out[0][2][k], out[1][2][k]
        assert (a is None) == (c is None) and (a is None or torch.equal(a, c)), k
    assert {s for _, s in seen} == {"attn_pre", "gate", "z", "out"}


def _geometry_cases():
    out = [(b, 128) for b in G.sweep_batches(128)] + [(b, 48) for b in G.idle_batches(48)]
    return out + [(b, 16) for b in G.one_tile_batches(16)]


@pytest.mark.parametrize("b,l_c", _geometry_cases(), ids=[f"lc{l}_b{b}" for b, l in _geometry_cases()])
def test_geometry_case_sees_every_mutation(b, l_c):
    case = G.sweep_case(b, l_c)
    _census(case)
    ref = G.oracle_grads(case)
    tiles, _, C = G.geometry(b, l_c)
    step = G.latent_ff_step(case)
    for tile, what in ((0, "first tile of sample 0"), (tiles - 1, "last real tile")):
        _require(case, f"lost tile {tile} ({what})", G.oracle_grads(case, tap=G.mutation_tap(case, "lost_tile", step=step, tile=tile)), ref)
    hid = 4 * case.kw["l_d"]
    c = max(C, 4) - 1           # without a cluster: the last of the chunks a C = 4 cluster would split
    lo, hi = hid * c // max(C, 4), hid * (c + 1) // max(C, 4)
    got = G.oracle_grads(case, tap=G.mutation_tap(case, "lost_member", step=step, tile=tiles - 1, lo=lo, hi=hi))
    _require(case, f"lost member {c} of C = {C} (hidden {lo}:{hi}) in tile {tiles - 1}", got, ref)
    if b > 1:
        got = G.oracle_grads(case, tap=G.mutation_tap(case, "sample_slip", step=G.latent_attn_step(case), s=b - 2))
        _require(case, f"sample slip {b - 2} -> {b - 1}", got, ref)


def test_gelu_case():
    case = G.sweep_case(5, 128, snn=False)
    _census(case)
    ref = G.oracle_grads(case)
    tiles = G.geometry(5, 128)[0]
    got = G.oracle_grads(case, tap=G.mutation_tap(case, "lost_tile", step=G.latent_ff_step(case), tile=tiles - 1))
    _require(case, "lost last tile", got, ref)


def test_shared_weights_case_sees_a_lost_use():
    """3 modalities, depth 3, tied layers: the self block runs 3x per layer and layers 1 and 2 share their blocks."""
    case = G.shared_case()
    _census(case)
    ref = G.oracle_grads(case)
    for layer in (0, 2):
        for use in (0, 2):
            got = G.oracle_grads(case, tap=G.mutation_tap(case, "lost_use", step=G.latent_attn_step(case, layer, use)))
            _require(case, f"lost use {use} of the layer-{layer} self block", got, ref)
    tiles = G.geometry(case.b, case.kw["l_c"])[0]
    got = G.oracle_grads(case, tap=G.mutation_tap(case, "lost_tile", step=G.latent_ff_step(case, 2), tile=tiles - 1))
    _require(case, "lost last tile in layer 2", got, ref)


@pytest.mark.parametrize("name", ["missing", "masked"])
def test_missing_and_masked_cases(name):
    case = G.missing_case() if name == "missing" else G.masked_case()
    _census(case)
    ref = G.oracle_grads(case)
    tiles = G.geometry(case.b, case.kw["l_c"])[0]
    got = G.oracle_grads(case, tap=G.mutation_tap(case, "lost_tile", step=G.latent_ff_step(case), tile=tiles - 1))
    _require(case, "lost last tile", got, ref)
    got = G.oracle_grads(case, tap=G.mutation_tap(case, "sample_slip", step=G.latent_attn_step(case), s=case.b - 2))
    _require(case, "sample slip", got, ref)


@pytest.mark.parametrize("name", list(G.STAGED))
def test_staged_dropout_case_sees_a_mask_slip(name):
    """Under random Bernoulli multipliers of the build's shapes (the GPU test uses the exported ones)."""
    kw = G.staged_kw(name)
    case = G.staged_case(name, G.random_drop(kw, 3))
    _census(case)
    ref = G.oracle_grads(case)
    for step in sorted(case.drop)[:2]:
        _require(case, f"dropout mask of block {step} shifted by one row", G.oracle_grads(case, drop=G.shift_mask(case.drop, step)), ref)
    tiles = G.geometry(case.b, case.kw["l_c"])[0]
    got = G.oracle_grads(case, tap=G.mutation_tap(case, "lost_tile", step=G.latent_ff_step(case), tile=tiles - 1))
    _require(case, "lost last tile", got, ref)


def test_cfg4_case_is_kink_free():
    _census(G.cfg4_case(2))
