"""CPU self-check of tests/test_gpu_train_fp64.py: the fp64 restatements of hn_surv_nll / hn_l1_adam_step equal the oracle; every bug
class of the two kernels -- a skipped tail or grid-stride round, a wrong bias correction / beta1 / step / sign(0) / grad_scale / eps
placement, unnormalised class weights, a label read one bin off, a dropped clamp gate, a sample slip -- moves some checked quantity
by SENSITIVITY x its bound; the Adam bound holds for torch's own fp32 Adam (it is not too tight); every survival case passes its
clamp census; and the oracle's fp32 path still reproduces the reference fixtures."""
import math

import pytest
import torch

import train_tail_cases as TT
from conftest import load_golden
from oracle import train_cpu as T

ADAM = TT.adam_cases()
SURV = TT.surv_cases() + [TT.bad_label_case()]


def _torch_adam(c):
    """torch.optim.Adam's single-tensor fp32 step on the case (the gradient of l1 * sum |p| added in fp32 by autograd's rule)."""
    p = torch.nn.Parameter(c.p.clone())
    p.grad = c.g * c.gs + c.l1 * torch.sign(c.p)
    opt = torch.optim.Adam([p], lr=c.lr, betas=(c.beta1, c.beta2), eps=c.eps, foreach=False, fused=False)
    opt.state[p] = {"step": torch.tensor(float(c.step - 1)), "exp_avg": c.m.clone(), "exp_avg_sq": c.v.clone()}
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


@pytest.mark.parametrize("case", ADAM, ids=[c.name for c in ADAM])
def test_adam_bound_holds_for_torch_fp32(case):
    ex = TT.adam_excess((case.p, case.g, case.m, case.v), _torch_adam(case), case.scalars(),
                        reg=float(case.l1) * float(case.p.abs().sum()))
    print(case.name, {k: f"{r:.3f}" for k, (r, _) in ex.items()})
    for k, (r, e) in ex.items():
        assert r <= 1.0, f"{case.name} {k}: torch's fp32 Adam is off by {e:.3e} = {r:.2f} x the bound"


@pytest.mark.parametrize("case", ADAM, ids=[c.name for c in ADAM])
def test_adam_model_is_the_oracle(case):
    sc = case.scalars()
    ref = TT.adam_ref64(case.p, case.g, case.m, case.v, **sc)
    got = TT.adam_model(case.p, case.g, case.m, case.v, **sc)
    bnd = TT.adam_bound(case.p, case.g, case.m, case.v, **sc)
    for a, b, lim in zip(got[:3], ref[:3], bnd):
        assert float(((a - b).abs() - 1e-6 * lim).max()) <= 0
    assert abs(got[3] - ref[3]) <= 1e-12 * max(abs(ref[3]), 1e-30)


@pytest.mark.parametrize("mutation", TT.ADAM_MUTATIONS)
def test_adam_mutation_is_caught(mutation):
    shifts = {c.name: TT.adam_shift(c, mutation) for c in ADAM}
    best = max(shifts, key=shifts.get)
    print(f"{mutation}: {shifts[best]:.2e} x the bound at {best}")
    assert shifts[best] >= TT.SENSITIVITY, f"{mutation}: largest shift {shifts[best]:.2e} x the bound"


def test_adam_cases_cover_the_issue():
    sizes = {c.p.numel() for c in ADAM}
    assert {1, 3, 5, 1023, 1025, 2 ** 20 - 1, 2 ** 20 + 1, 2 ** 20 + 1024} <= sizes
    assert {c.l1 for c in ADAM} == {0.0, 3e-4} and {c.gs for c in ADAM} == {1.0, 0.5, 0.125}
    assert {c.step for c in ADAM} == {1, 2, 10, 1000, 100000} and {c.beta1 for c in ADAM} == {0.85, 0.95}
    assert TT.adam_blocks(2 ** 20 + 1024) == TT.ADAM_BLOCKS and (2 ** 20 + 1024) // 4 > TT.ADAM_BLOCKS * TT.ADAM_THREADS
    c = ADAM[-1]
    assert (c.p == 0).any() and (torch.signbit(c.p) & (c.p == 0)).any() and (c.g == 0).any()
    gt = c.g.double() * c.gs + c.l1 * torch.sign(c.p.double())
    assert ((gt != 0) & (gt.abs() < 1e-22)).any(), "no gradient whose square is under the fp32 denormal range"
    assert ((c.v.double().sqrt() / math.sqrt(1 - c.beta2 ** c.step)) < 1e-3 * c.eps).any(), "no element where eps dominates"


def test_cfg2_flat_numel():
    from healnet_amd import HealNet
    model = HealNet(n_modalities=2, channel_dims=[2000, 3], num_spatial_axes=[1, 2], out_dims=4)
    assert sum((p.numel() + 3) // 4 * 4 for p in model.parameters()) == TT.CFG2_FLAT_NUMEL


@pytest.mark.parametrize("case", SURV, ids=[c.name for c in SURV])
def test_surv_case_census_and_model(case):
    worst = TT.census(case)
    print(f"{case.name}: clamp census margin {worst:.1f}")
    assert worst >= 1.0, f"{case.name}: an A / H / B lies within {TT.CENSUS} x its fp32 deviation of eps"
    ref = TT.surv_oracle(case)
    got = TT.surv_model(case.logits, case.y_safe, case.c, case.w, case.gs)
    for k in ref:
        assert torch.allclose(got[k], ref[k], rtol=1e-12, atol=1e-300), k
    e32 = TT.row_errors(TT.surv_oracle(case, torch.float32), ref, case.bad)
    for k, e in e32.items():
        assert TT.K * float(e.max()) <= TT.SURV_CEIL, f"{case.name} {k}: the fp32 oracle's error puts the bound above the ceiling"


@pytest.mark.parametrize("mutation", TT.SURV_MUTATIONS)
def test_surv_mutation_is_caught(mutation):
    shifts = {c.name: TT.surv_shift(c, mutation) for c in SURV if not c.bad}
    best = max(shifts, key=shifts.get)
    print(f"{mutation}: {shifts[best] / TT.SURV_CEIL:.2e} x the ceiling at {best}")
    assert shifts[best] >= TT.SENSITIVITY * TT.SURV_CEIL


def test_surv_cases_cover_the_issue():
    assert {c.logits.shape[1] for c in SURV} >= {1, 2, 4, 7, 16, 63, 64}
    assert {c.logits.shape[0] for c in SURV} >= {1, 255, 256, 257, 1000, 4096}
    assert any(c.w is None for c in SURV) and any(c.w is not None for c in SURV)
    assert any(bool((c.c == 1).all()) for c in SURV) and any(bool((c.c == 0).all()) for c in SURV)
    assert any(bool(((c.c > 0) & (c.c < 1)).any()) for c in SURV)
    assert all(bool((c.y_safe == 0).any()) and bool((c.y == c.logits.shape[1] - 1).any()) for c in SURV if len(c.y) > 1)
    for v in (40.0, 90.0):
        assert any(bool((c.logits == v).any()) and bool((c.logits == -v).any()) for c in SURV)
    assert any(c.gs != 1.0 for c in SURV)


def test_oracle_fp32_path_still_matches_fixtures(manifest):
    """The fp64 wrappers call oracle/train_cpu.py unchanged; its fp32 path still reproduces g7_* (as test_oracle_golden.py)."""
    g = load_golden("g7_surv_nll")
    meta = manifest["g7_surv_nll"]
    for case in meta["cases"]:
        t = case["tag"]
        loss, dl, _, _ = T.surv_nll(g[t + "logits"], g[t + "y"], g[t + "c"], g[t + "weights"] if case["weighted"] else None,
                                    alpha=meta["alpha"], eps=meta["eps"])
        assert abs(float(loss) - float(g[t + "loss"])) <= 1e-6 * max(1.0, abs(float(g[t + "loss"])))
        assert torch.allclose(dl, g[t + "dlogits"], rtol=1e-5, atol=1e-7)
