"""GPU: every parameter gradient of the fused backward -- the latent backward chains and their clusters (bchain.hip), the per-block
launches, attention_bwd.hip / backward.hip, the batched weight-gradient products and their fixed-order reduce, the x6 TN product of
dKV^T z, staged shapes, dropout -- against the fp64 oracle, per tensor and per slice (tests/grad_cases.py).

Yardstick (tests/long_context_cases.py's, unchanged): per slice, the HIP error against fp64 must be <= K x the fp32 oracle's error on
the same case, or under FLOOR["grad"], whichever is larger; that bound must itself stay under CEIL["grad"].  The references run
through torch on the GPU.  The cases are kink-free (grad_cases.repair) and tests/test_grad_sensitivity.py proves on the CPU that a
lost tile, a lost cluster member, a sample slip, a lost use of a shared block and a shifted dropout mask each move some slice by
more than SENSITIVITY x CEIL.

Measured on an MI355X: the largest HIP / fp32-oracle error ratio over every tensor and slice of a case (K = 8 holds with room on
every route; two runs, whose host-built cases differed in a few nudged bias columns; the largest HIP error of any slice was 9.7e-7,
so FLOOR = 2e-5 is the bound that applies nearly everywhere):
  cluster sweep l_c = 128   b = 1 / 3 / 8 (C = 4) 2.33 / 1.62 / 1.31;  b = 9 / 16 (C = 2) 2.56 / 2.80;  b = 17 (no cluster) 1.80 - 2.49
  idle members l_c = 48     b = 3 / 22 / 43 (9 -> 16, 66 -> 72, 129 -> 136 tiles) 1.84 / 2.72 / 3.18
  one tile l_c = 16         b = 1 / 5 2.71 / 1.85
  shared (tied, 3 uses)     2.08;  missing modality 2.72;  masked 1.83;  GELU 1.54;  staged + dropout brca 2.57, kirp 3.23
  cfg4 step (GraphedStep)   1.01;  HN_NO_X6_GEMM 1.59;  HN_FORCE_X6_GEMM (b = 1) 1.55
  HN_NO_BCHAIN              1.70 / 1.45 - 4.48 / 1.80 (l_c = 128 b = 3 / 9, l_c = 48 b = 3)
  HN_NO_CHAIN_CLUSTER       1.25 - 3.20 over the sweep and l_c = 48 b = 3
  route taken               the default route's bits differ from HN_NO_CHAIN_CLUSTER's at every C > 1 case, equal at b = 17
A scratch build whose backward chain (bchain.hip) skipped the last row tile of every sample failed every non-route case here, by
1.2e6 - 3.8e9 x the fp32 oracle's error.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import grad_cases as G
import long_context_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_ENVS = ("HN_NO_BCHAIN", "HN_NO_CHAIN_CLUSTER", "HN_NO_X6_GEMM", "HN_FORCE_X6_GEMM")


def _dev(ins):
    return [None if t is None else t.float().to(DEV) for t in ins]


def hip_grads(case):
    """Forward + fused backward of the build on the case -> {canonical key: gradient} (cpu)."""
    import healnet_amd as hn
    model = hn.HealNet(**case.kw).train()
    model.load_state_dict(case.sd, strict=True)
    model.to(DEV)
    y = model(_dev(case.ins), mask=None if case.mask is None else case.mask.to(DEV))
    (y * case.dl.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}


def step_grads(case):
    """The bench's step route: GraphedStep with surv_nll_loss, gradients read from the flat buffer."""
    import healnet_amd as hn
    model = hn.HealNet(**case.kw).train()
    model.load_state_dict(case.sd, strict=True)
    model.to(DEV)
    flat = hn.train.flatten_parameters(model)
    step = hn.train.GraphedStep(model, lambda logits, y, c: hn.train.surv_nll_loss(logits, y, c).loss)
    y, c = case.surv
    step(_dev(case.ins), (y.to(DEV), c.to(DEV)))
    step(_dev(case.ins), (y.to(DEV), c.to(DEV)))     # a replay of the captured graph: the gradients are zeroed, then written again
    torch.cuda.synchronize()
    assert step.captures == 1
    return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}


_REFS = {}


def refs(case):
    """(fp64, fp32) oracle gradients of the case, once per case object."""
    if id(case) not in _REFS:
        _REFS[id(case)] = (case, G.oracle_grads(case, device=DEV), G.oracle_grads(case, device=DEV, dtype=torch.float32))
    return _REFS[id(case)][1:]


def check(case, got, what):
    """Every canonical parameter, whole and per slice, against the yardstick; prints the largest ratio and error."""
    g64, g32 = refs(case)
    g64 = {k: v.cpu() for k, v in g64.items()}
    g32 = {k: v.cpu() for k, v in g32.items()}
    assert set(got) == set(g64), (sorted(set(got) ^ set(g64)))[:8]
    scale = G.grad_scale(g64)
    worst_ratio, worst_err, fails = 0.0, (0.0, ""), []
    for k in g64:
        assert torch.isfinite(got[k]).all(), f"{what}: non-finite gradient {k}"
        e32 = {lab: e for lab, e, _ in G.slice_errors(case, k, g32[k], g64[k], scale)}
        for lab, e, zero in G.slice_errors(case, k, got[k], g64[k], scale):
            bound = max(LC.K * e32[lab], LC.FLOOR["grad"])
            if bound > LC.CEIL["grad"]:
                fails.append(f"{k}[{lab}]: the fp32 oracle's own error {e32[lab]:.3e} puts the bound above {LC.CEIL['grad']:.0e}")
            if e > bound:
                fails.append(f"{k}[{lab}]{' (zero slice)' if zero else ''}: {e:.3e} > {bound:.2e} (fp32 oracle {e32[lab]:.3e})")
            if e32[lab] > 0:
                worst_ratio = max(worst_ratio, e / e32[lab])
            worst_err = max(worst_err, (e, f"{k}[{lab}]"))
    print(f"{what}: largest HIP / fp32-oracle ratio {worst_ratio:.2f}, largest HIP error {worst_err[0]:.2e} at {worst_err[1]}")
    assert not fails, f"{what}: {len(fails)} slices out of bound:\n  " + "\n  ".join(fails[:12])


GEOMETRY = ([(b, 128) for b in G.sweep_batches(128)] + [(b, 48) for b in G.idle_batches(48)] +
            [(b, 16) for b in G.one_tile_batches(16)])


@pytest.mark.parametrize("b,l_c", GEOMETRY, ids=[f"lc{l}_b{b}" for b, l in GEOMETRY])
def test_cluster_geometry_vs_fp64(b, l_c):
    """tab 1 x 300 + bag 40 x 64, depth 2: C = 4 / 2 / no cluster, idle members of a rounded grid, one tile on an 8-tile grid."""
    case = G.sweep_case(b, l_c)
    check(case, hip_grads(case), f"{case.name} (tiles, gtiles, C) = {G.geometry(b, l_c)}")


@pytest.mark.parametrize("name", ["shared", "missing", "masked", "gelu"])
def test_model_variants_vs_fp64(name):
    """Weight tying with the self block used 3x per layer (aliases summed); a None modality; a key mask; the GELU gate."""
    case = {"shared": G.shared_case, "missing": G.missing_case, "masked": G.masked_case,
            "gelu": lambda: G.sweep_case(5, 128, snn=False)}[name]()
    check(case, hip_grads(case), case.name)


@pytest.mark.parametrize("name", list(G.STAGED))
def test_staged_dropout_vs_fp64(name):
    """The reference's tuned TCGA shapes (zero-padded staged chains, EXT) with both dropouts, under the build's exported masks."""
    import healnet_amd as hn
    from test_gpu_dropout import _oracle_masks
    kw = G.full_kw(G.staged_kw(name))
    b = 3
    model = hn.HealNet(**kw).train()
    seed, offset = torch.initial_seed(), model._rng_offset + 1        # what the next training forward draws
    n_tokens = [1 if s is None else s[0] for s in G.STAGED_SHAPES]
    drop = _oracle_masks(hn, model, kw, b, n_tokens, seed, offset, [True, True])
    case = G.staged_case(name, drop, b)
    model.load_state_dict(case.sd, strict=True)
    model.to(DEV)
    assert model.runs_staged()
    y = model(_dev(case.ins))
    assert model._last_rng == (seed, offset)
    (y * case.dl.float().to(DEV)).sum().backward()
    got = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    check(case, got, case.name)


def test_cfg4_training_step_vs_fp64():
    """omic 1 x 2000 + bag 4096 x 768, depth 3, b = 2 through GraphedStep + surv_nll_loss: the bench's step route, the x6 TN
    gradient of the bag's K/V projection at the 8192-row gate."""
    case = G.cfg4_case(2)
    check(case, step_grads(case), case.name + " GraphedStep")


# ---- route variants, each in a fresh process
ROUTES = {
    "HN_NO_BCHAIN": [("sweep", 3, 128), ("sweep", 9, 128), ("sweep", 3, 48)],
    "HN_NO_CHAIN_CLUSTER": [("sweep", b, 128) for b in G.sweep_batches(128)] + [("sweep", 3, 48)],
    "HN_NO_X6_GEMM": [("cfg4", 2, 0)],
    "HN_FORCE_X6_GEMM": [("cfg4", 1, 0)],
}

_ROUTE_SCRIPT = """
import sys, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
import grad_cases as G
import test_gpu_grad_fp64 as T
out = {{}}
for kind, b, l_c in {runs!r}:
    case = G.sweep_case(b, l_c) if kind == "sweep" else G.cfg4_case(b)
    out[(kind, b, l_c)] = T.hip_grads(case) if kind == "sweep" else T.step_grads(case)
torch.save(out, sys.argv[1])
"""


@functools.lru_cache(maxsize=None)
def _route_run(route, path):
    script = os.path.join(path, f"{route}.py")
    with open(script, "w") as f:
        f.write(_ROUTE_SCRIPT.format(root=ROOT, runs=ROUTES[route]))
    env = {k: v for k, v in os.environ.items() if k not in ROUTE_ENVS}
    env[route] = "1"
    out = os.path.join(path, f"{route}.pt")
    r = subprocess.run([sys.executable, script, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def route_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("routes"))


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_variants_vs_fp64(route, route_dir):
    """HN_NO_BCHAIN (per-block launches), HN_NO_CHAIN_CLUSTER (per-tile grids), HN_NO_X6_GEMM (fp32-MFMA TN product at 8192 rows),
    HN_FORCE_X6_GEMM (the x6 route at 4096 rows), each forced in a fresh process."""
    got = _route_run(route, route_dir)
    for kind, b, l_c in ROUTES[route]:
        case = G.sweep_case(b, l_c) if kind == "sweep" else G.cfg4_case(b)
        check(case, got[(kind, b, l_c)], f"{case.name} {route}")


@functools.lru_cache(maxsize=None)
def _default_sweep(b, l_c):
    return hip_grads(G.sweep_case(b, l_c))


def test_route_taken_follows_the_geometry(route_dir):
    """The cluster launch changes the summation order (members split the hidden chunks and exchange partial tiles), so the default
    route's gradients differ in their bits from the per-tile route's exactly where the restatement says C > 1."""
    got = _route_run("HN_NO_CHAIN_CLUSTER", route_dir)
    for kind, b, l_c in ROUTES["HN_NO_CHAIN_CLUSTER"]:
        mine = _default_sweep(b, l_c)
        same = all(torch.equal(mine[k], got[(kind, b, l_c)][k]) for k in mine)
        C = G.geometry(b, l_c)[2]
        print(f"l_c = {l_c} b = {b}: C = {C}, bit-equal to the per-tile route: {same}")
        assert same == (C == 1), f"l_c = {l_c} b = {b}: C = {C} but bit-equal = {same}"
