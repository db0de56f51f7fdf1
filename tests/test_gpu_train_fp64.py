"""GPU: the training-step tail (healnet_amd/csrc/train.hip) against fp64, per element -- hn_surv_nll per tensor and per sample
row, hn_l1_adam_step per element of p / exp_avg / exp_avg_sq and its reg_loss, through the C ABI, through FusedL1Adam under
OneCycleLR, at the production size (cfg4 b = 8, eager and GraphedStep), with frozen and tied parameters, across a checkpoint.

Yardsticks (tests/train_tail_cases.py): the survival loss meets max(K x the fp32 oracle's error, SURV_FLOOR) per tensor and row,
under SURV_CEIL; each Adam step meets the per-element first-order rounding bound of that module's docstring (x ADAM_SAFETY), fed
the step's own fp32 inputs, and reg_loss a summation bound.  Every multi-step check restarts from a snapshot of the step's inputs,
so fp32 rounding cannot compound into a drifting trajectory.  tests/test_train_tail_sensitivity.py proves on the CPU that each
bug class the issue names moves some checked quantity by SENSITIVITY x its bound and that torch's own fp32 Adam meets the bound.

Measured on an MI355X (largest error / bound of any element, row or step; 1.0 fails):
  hn_surv_nll, 27 cases          0.125 (b = 1, K = 7 survival, at 1.0 x the fp32 oracle's own error); every other case <= 0.07, largest
                                 error 2.8e-7 of the tensor's scale, so SURV_FLOOR = 4e-6 is the bound that applies nearly everywhere
  hn_l1_adam_step, 9 sizes       p 0.03 - 0.25, exp_avg 0.02 - 0.23, exp_avg_sq 0.06 - 0.19, reg_loss <= 0.013
  OneCycleLR, 240 steps          0.247;   cfg4 b = 8, 3 steps eager and graphed: 0.250, loss error 2.1e-7 (fp32 oracle 1.0e-7)
torch's own fp32 Adam reaches 0.25 of the same bound on the CPU (tests/test_train_tail_sensitivity.py).
A scratch build whose l1_adam_kernel stopped after its first grid-stride round failed n = 2^20 + 1024, the cfg2 buffer and both cfg4
runs by 2.1e5 - 5.1e5 x the bound.  A scratch build whose surv_nll_kernel read sample i + 1's logits failed every case with b > 1
(the failures inspected: 1e4 - 2e5 x the bound).
"""
import ctypes as C

import pytest
import torch

import train_tail_cases as TT
from oracle import train_cpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hn():
    import healnet_amd
    return healnet_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------------------
# (a) hn_surv_nll
# ------------------------------------------------------------------------------------------------------------------------------
def hip_surv(case, K=None):
    from healnet_amd import _capi
    lg = case.logits.to(DEV).contiguous()
    b, nb = lg.shape
    y, c = case.y.to(DEV).contiguous(), case.c.to(DEV).contiguous()
    w = None if case.w is None else case.w.to(DEV).contiguous()
    loss = torch.full((1,), 123.0, device=DEV)
    dl, hz, sv = (torch.full_like(lg, 123.0) for _ in range(3))
    rk = torch.full((b,), 123.0, device=DEV)
    rc = _capi.lib().hn_surv_nll(lg.data_ptr(), y.data_ptr(), c.data_ptr(), None if w is None else w.data_ptr(), b,
                                 nb if K is None else K, TT.ALPHA, TT.EPS, case.gs, loss.data_ptr(), dl.data_ptr(), hz.data_ptr(),
                                 sv.data_ptr(), rk.data_ptr(), C.c_void_p(_stream()))
    torch.cuda.synchronize()
    return rc, dict(loss=loss.cpu(), dlogits=dl.cpu(), hazards=hz.cpu(), survival=sv.cpu(), risk=rk.cpu())


def check_surv(case, got, what):
    ref64, ref32 = TT.surv_oracle(case), TT.surv_oracle(case, torch.float32)
    e, e32 = TT.row_errors(got, ref64, case.bad), TT.row_errors(ref32, ref64, case.bad)
    fails, worst = [], (0.0, "", 0.0)
    for k in e:
        bound = torch.clamp(TT.K * e32[k], min=TT.SURV_FLOOR)
        if float(bound.max()) > TT.SURV_CEIL:
            fails.append(f"{k}: the fp32 oracle's error puts the bound at {float(bound.max()):.2e} > {TT.SURV_CEIL:.0e}")
        bad = (~(e[k] <= bound)).nonzero().view(-1)         # (NaN fails too)
        if len(bad):
            i = int(bad[0])
            fails.append(f"{k}: {len(bad)} rows out of bound, first row {i}: {float(e[k][i]):.3e} > {float(bound[i]):.2e}")
        r = e[k] / bound
        if bool(torch.isfinite(r).all()):
            worst = max(worst, (float(r.max()), k, float(e[k].max())))
    print(f"{what}: largest error / bound {worst[0]:.3f} ({worst[1]}: {worst[2]:.2e})")
    assert not fails, f"{what}:\n  " + "\n  ".join(fails)


SURV = TT.surv_cases()


@pytest.mark.parametrize("case", SURV, ids=[c.name for c in SURV])
def test_surv_nll_vs_fp64(case):
    rc, got = hip_surv(case)
    assert rc == 0
    check_surv(case, got, case.name)


def test_surv_nll_bad_labels_stay_in_their_rows():
    """y = -1 and y = K: the loss and exactly those rows of dlogits are NaN; every other row meets the bound."""
    case = TT.bad_label_case()
    rc, got = hip_surv(case)
    assert rc == 0
    assert torch.isnan(got["loss"]).all()
    nan_rows = torch.isnan(got["dlogits"]).any(1).nonzero().view(-1).tolist()
    assert nan_rows == sorted(case.bad) and torch.isnan(got["dlogits"][case.bad]).all()
    check_surv(case, got, case.name)


def test_surv_nll_autograd_route_vs_fp64(hn):
    """surv_nll_loss (grad_scale 1 inside, the upstream gradient applied by autograd) on a K = 64 case."""
    case = TT.surv_case(257, 64, weighted=True, cens="mixed", sat=True, seed=5)
    lg = case.logits.to(DEV).requires_grad_(True)
    out = hn.train.surv_nll_loss(lg, case.y.to(DEV), case.c.to(DEV), weights=case.w.to(DEV), alpha=TT.ALPHA, eps=TT.EPS)
    out.loss.backward()
    got = dict(loss=out.loss.detach().reshape(1).cpu(), dlogits=lg.grad.cpu(), hazards=out.hazards.cpu(), survival=out.survival.cpu(),
               risk=out.risk.cpu())
    check_surv(case, got, "autograd " + case.name)


def test_surv_nll_rejects_65_bins():
    from healnet_amd import _capi
    case = TT.surv_case(4, 64, seed=3)
    case.logits = torch.zeros(4, 65)
    rc, got = hip_surv(case, K=65)
    assert rc == _capi.HN_E_SHAPE
    assert (got["loss"] == 123.0).all() and (got["dlogits"] == 123.0).all()      # nothing was written


# ------------------------------------------------------------------------------------------------------------------------------
# (b) hn_l1_adam_step through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def hip_adam(p, g, m, v, step, lr, beta1, beta2, eps, l1, gs):
    """One hn_l1_adam_step on device copies -> (p', m', v'), reg_loss."""
    from healnet_amd import _capi
    lib = _capi.lib()
    p, g, m, v = (t.to(DEV).float().contiguous().clone() for t in (p, g, m, v))
    reg = torch.full((1,), -1.0, device=DEV)
    ws = torch.empty(lib.hn_l1_adam_workspace_bytes(), dtype=torch.uint8, device=DEV)
    rc = lib.hn_l1_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), l1, gs, lr, beta1, beta2, eps, step,
                             reg.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(_stream()))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (p, m, v), float(reg)


def check_adam(before, after, sc, reg, what):
    ex = TT.adam_excess(before, after, sc, reg=reg)
    print(f"{what}: " + ", ".join(f"{k} {r:.3f} x bound ({e:.1e})" for k, (r, e) in ex.items()))
    bad = {k: v for k, v in ex.items() if not v[0] <= 1.0}
    assert not bad, f"{what}: out of bound {bad}"
    return max(r for r, _ in ex.values())


ADAM = TT.ADAM_SIZES + [TT.CFG2_FLAT_NUMEL]


@pytest.mark.parametrize("i", range(len(ADAM)), ids=[f"n{n}" for n in ADAM])
def test_l1_adam_step_vs_fp64(i):
    """Every element of p / exp_avg / exp_avg_sq and reg_loss; tails of 1 - 3 elements, one workgroup, the last element of the
    first grid-stride round, the start of a second one, and the cfg2 model's flat buffer (9.6 M elements, 3 rounds)."""
    case = TT.adam_case(i, ADAM[i])
    sc = case.scalars()
    after, reg = hip_adam(case.p, case.g, case.m, case.v, **sc)
    before = tuple(t.to(DEV) for t in (case.p, case.g, case.m, case.v))
    check_adam(before, after, sc, reg, case.name)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) FusedL1Adam under OneCycleLR, every step against a one-step oracle fed that step's snapshot
# ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(37, 5), (4,), (1,), (129,), (16, 16), (3, 3, 3)]


class _Holder(torch.nn.Module):
    def __init__(self, shapes, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=gen) * 0.1) for s in shapes])


def _grads(model, t, seed=0):
    """Fresh gradients of step t: magnitudes 1e-7 .. 1e-1, some exact zeros; written into each trainable .grad (the flat slots)."""
    gen = torch.Generator().manual_seed(10007 * seed + t)
    for p in model.parameters():
        if not p.requires_grad:
            continue
        gg = torch.randn(p.shape, generator=gen) * torch.pow(10.0, torch.rand(p.shape, generator=gen) * 6 - 7)
        gg[torch.rand(p.shape, generator=gen) < 0.05] = 0.0
        p.grad.copy_(gg.to(DEV))


def _snap(flat, opt):
    return tuple(t.detach().clone() for t in (flat.params, flat.grads, opt.exp_avg, opt.exp_avg_sq))


def _scalars(opt):
    g = opt.param_groups[0]
    return dict(step=opt._steps + 1, lr=float(g["lr"]), beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]),
                l1=float(g["l1"]), gs=float(g["grad_scale"]))


def test_fused_adam_one_cycle_every_step_vs_fp64(hn):
    model = _Holder(SHAPES).to(DEV)
    flat = hn.train.flatten_parameters(model)
    opt = hn.train.FusedL1Adam(flat, lr=1e-4, l1=3e-4, grad_scale=0.5)
    steps = 240
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=steps)
    worst = 0.0
    b1s = []
    for t in range(steps):
        opt.zero_grad()
        _grads(model, t)
        before, sc = _snap(flat, opt), _scalars(opt)
        opt.step()
        b1s.append(sc["beta1"])
        worst = max(worst, check_adam(before, (flat.params, opt.exp_avg, opt.exp_avg_sq), sc, float(opt.reg_loss), f"step {t + 1}"))
        sched.step()
    assert min(b1s) == pytest.approx(0.85) and max(b1s) == pytest.approx(0.95)
    print(f"OneCycle {steps} steps: largest error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# (d) production size: cfg4 b = 8, eager and GraphedStep
# ------------------------------------------------------------------------------------------------------------------------------
def _check_loss(logits, y, c, loss, what):
    l64 = float(T.surv_nll(logits.double().cpu(), y.cpu(), c.cpu())[0])
    l32 = float(T.surv_nll(logits.float().cpu(), y.cpu(), c.cpu())[0])
    e, e32 = abs(float(loss) - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    bound = max(TT.K * e32, TT.SURV_FLOOR)
    print(f"{what}: loss error {e:.2e} (fp32 oracle {e32:.2e})")
    assert bound <= TT.SURV_CEIL and e <= bound, (what, e, bound)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_cfg4_training_steps_vs_fp64(hn, graphed):
    torch.manual_seed(0)
    kw = dict(n_modalities=2, channel_dims=[2000, 768], num_spatial_axes=[1, 1], out_dims=4)
    model = hn.HealNet(**kw).train().to(DEV)
    gen = torch.Generator().manual_seed(4321)
    b = 8
    ins = [torch.rand(b, *s, generator=gen).to(DEV) for s in [(1, 2000), (4096, 768)]]
    y = torch.randint(0, 4, (b,), generator=gen).to(DEV)
    c = torch.randint(0, 2, (b,), generator=gen).to(DEV)
    flat = hn.train.flatten_parameters(model)
    opt = hn.train.FusedL1Adam(flat, lr=1e-4, l1=1e-4)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=20)
    gstep = hn.train.GraphedStep(model, lambda lg, yy, cc: hn.train.surv_nll_loss(lg, yy, cc).loss) if graphed else None
    for t in range(3):
        if graphed:
            loss, logits = gstep(ins, (y, c))
        else:
            opt.zero_grad()
            logits = model(list(ins))
            out = hn.train.surv_nll_loss(logits, y, c)
            out.loss.backward()
            loss, logits = out.loss.detach(), logits.detach()
        torch.cuda.synchronize()
        _check_loss(logits, y, c, loss, f"step {t + 1}")
        before, sc = _snap(flat, opt), _scalars(opt)
        opt.step()
        check_adam(before, (flat.params, opt.exp_avg, opt.exp_avg_sq), sc, float(opt.reg_loss), f"cfg4 step {t + 1}")
        sched.step()
    if graphed:
        assert gstep.captures == 1
        gstep.close()


# ------------------------------------------------------------------------------------------------------------------------------
# (e) frozen and tied parameters
# ------------------------------------------------------------------------------------------------------------------------------
class _Tied(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(2)
        self.a = torch.nn.Parameter(torch.randn(10, 7, generator=gen) * 0.1)
        self.b = torch.nn.Parameter(torch.randn(33, generator=gen) * 0.1)
        self.c = torch.nn.Parameter(torch.randn(5, 5, generator=gen) * 0.1)
        self.c_again = self.c                                  # tied: one parameter under two names
        self.d = torch.nn.Parameter(torch.randn(6, generator=gen) * 0.1)


def _slot(flat, p):
    return next(off for q, off in zip(flat.views, flat.offsets) if q is p)


def test_frozen_and_tied_parameters_vs_torch_adam(hn):
    """Against torch.optim.Adam + zero_grad() (set_to_none) + calc_reg_loss: b frozen after flattening keeps p / exp_avg /
    exp_avg_sq bit-identical with l1 > 0 and with l1 = 0 after nonzero moments, then resumes with its own update count; d, frozen
    before flattening, counts in reg_loss; the tied c is counted once."""
    l1, lr = 3e-4, 1e-3
    model = _Tied().to(DEV)
    model.d.requires_grad_(False)
    ref = {k: p.detach().clone().requires_grad_(p.requires_grad) for k, p in model.named_parameters()}
    assert set(ref) == {"a", "b", "c", "d"}
    flat = hn.train.flatten_parameters(model)
    opt = hn.train.FusedL1Adam(flat, lr=lr, l1=l1)
    ropt = torch.optim.Adam([ref[k] for k in ("a", "b", "c")], lr=lr, foreach=False)
    sl = slice(_slot(flat, model.b), _slot(flat, model.b) + model.b.numel())
    plan = [(l1, True)] * 3 + [(l1, False)] * 3 + [(0.0, False)] * 2 + [(l1, True)] * 3
    held = None
    for t, (lam, b_on) in enumerate(plan):
        model.b.requires_grad_(b_on)
        ref["b"].requires_grad_(b_on)
        opt.param_groups[0]["l1"] = lam
        opt.zero_grad()
        ropt.zero_grad()
        gen = torch.Generator().manual_seed(t)
        want_reg = lam * float(sum(p.detach().abs().sum() for p in ref.values()))
        for k in ("a", "b", "c"):
            gg = (torch.randn(ref[k].shape, generator=gen) * 1e-2).to(DEV)
            if ref[k].requires_grad:
                getattr(model, k).grad.copy_(gg)
                ref[k].grad = gg + lam * torch.sign(ref[k].detach())
        opt.step()
        ropt.step()
        assert float(opt.reg_loss) == pytest.approx(want_reg, rel=1e-5, abs=1e-12), t
        if not b_on:
            now = (model.b.detach().clone(), opt.exp_avg[sl].clone(), opt.exp_avg_sq[sl].clone())
            if held is None:
                assert float(now[1].abs().max()) > 0 and float(now[2].abs().max()) > 0
            else:
                for x, h in zip(now, held):
                    assert torch.equal(x, h), f"step {t + 1}: a frozen parameter or its moments moved"
            held = now
        for k in ("a", "b", "c"):
            diff = float((getattr(model, k).detach() - ref[k].detach()).abs().max())
            assert diff <= 1e-3 * lr, f"step {t + 1}: {k} is {diff:.2e} away from torch.optim.Adam"
            s = ropt.state[ref[k]]
            if s:
                o = _slot(flat, getattr(model, k))
                n = ref[k].numel()
                assert torch.allclose(opt.exp_avg[o:o + n], s["exp_avg"].reshape(-1), rtol=1e-5, atol=1e-12)
                assert torch.allclose(opt.exp_avg_sq[o:o + n], s["exp_avg_sq"].reshape(-1), rtol=1e-5, atol=1e-16)
    model.d.requires_grad_(True)
    with pytest.raises(RuntimeError, match="flatten_parameters"):
        opt.step()


# ------------------------------------------------------------------------------------------------------------------------------
# (f) checkpoint round trip
# ------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_is_bit_identical(hn):
    """state_dict() of FusedL1Adam (and the scheduler) saved mid-schedule, reloaded into a fresh model / optimizer: the rest of
    the run equals the uninterrupted one bit for bit -- a view frozen for a while before the checkpoint included."""
    import io

    def make(sd=None):
        model = _Holder(SHAPES, seed=1).to(DEV)
        if sd is not None:
            model.load_state_dict(sd)
        flat = hn.train.flatten_parameters(model)
        opt = hn.train.FusedL1Adam(flat, lr=1e-4, l1=3e-4, grad_scale=0.5)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=40)
        return model, flat, opt, sched

    def run(model, opt, sched, ts):
        for t in ts:
            model.ps[3].requires_grad_(not 2 <= t < 5)
            opt.zero_grad()
            _grads(model, t, seed=1)
            opt.step()
            sched.step()

    model, flat, opt, sched = make()
    run(model, opt, sched, range(6))
    buf = io.BytesIO()
    torch.save({"model": model.state_dict(), "opt": opt.state_dict(), "sched": sched.state_dict()}, buf)
    run(model, opt, sched, range(6, 12))
    buf.seek(0)
    ck = torch.load(buf, map_location=DEV)
    model2, flat2, opt2, sched2 = make(ck["model"])
    opt2.load_state_dict(ck["opt"])
    sched2.load_state_dict(ck["sched"])
    run(model2, opt2, sched2, range(6, 12))
    assert opt2._steps == opt._steps == 12
    for a, b in ((flat.params, flat2.params), (opt.exp_avg, opt2.exp_avg), (opt.exp_avg_sq, opt2.exp_avg_sq), (opt.reg_loss, opt2.reg_loss)):
        assert torch.equal(a, b)
