"""GPU: the attention cores at production context lengths -- every token, every sample -- against the fp64 oracle.

The cases (tests/long_context_cases.py) sharpen the queries of the long-context cross blocks and put needles on the edges of every
token split of the forward and backward plans, so that a skipped or doubled tile, a short last split, a wrong merge weight, a
per-sample stride slip or a leaking masked token moves the output far beyond the bound checked here
(tests/test_long_context_sensitivity.py proves that on the CPU for every case).

Yardstick (tests/test_gpu_x6.py's): against the fp64 oracle, the HIP error must be <= K x the fp32 oracle's error on the same inputs,
or under FLOOR, whichever is larger; that bound must itself stay under CEIL.  The references run through torch on the GPU (fp64 and
fp32 oracle), which keeps the host cost of the file small.

Measured on an MI355X (HIP error / fp32-oracle error, both against fp64; K = 8 holds with room on every route):
  cfg2 image fp32 core, b = 1 / 2 / 8 / 32, depth 1 and 3   embeddings 0.36 - 0.82, logits 0.33 - 1.46 (errors 1.4e-7 .. 9.2e-7)
  attention weights, row-relative                         2.43 (9.1e-5 against 3.7e-5: the sharpened scores make even the fp32
                                                          oracle's P error large, hence CEIL["probs"] = 1e-3)
  cfg4 bag, default route b = 1 / 8                       0.63 - 1.38;  forced x6: 0.63 - 1.38;  forced fp32 MFMA: 0.75 - 1.68
  masked-needle bag                                       0.91 / 1.24
  cfg3 volume, 4 frames (N = 200 704)                     0.60 / 0.73
  gradients of the long-context cross blocks, b = 2       cfg2 0.31 - 1.51, cfg4 0.58 - 1.72
  bf16x3 embeddings 5.1e-6 - 6.4e-6 (tolerance 1e-3);  bf16 image contribution 6.5e-3 - 7.2e-3 (tolerance 2e-2)
"""
import os
import subprocess
import sys

import pytest
import torch

import long_context_cases as LC
from oracle import healnet_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hn():
    import healnet_amd
    return healnet_amd


def _model(hn, case, core_precision="fp32", train=False):
    model = hn.HealNet(**case.kw, core_precision=core_precision).train(train)
    model.load_state_dict(case.sd, strict=True)
    return model.to(DEV)


def _dev(ins):
    return [None if t is None else t.float().to(DEV) for t in ins]


def _check(got, ref64, ref32, kind, what):
    """err(HIP) <= max(K * err(fp32 oracle), FLOOR[kind]) <= CEIL[kind]; returns the measured ratio for the record."""
    e, e32 = LC.err(got, ref64), LC.err(ref32, ref64)
    bound = max(LC.K * e32, LC.FLOOR[kind])
    print(f"{what}: HIP {e:.3e}  fp32 oracle {e32:.3e}  ratio {e / max(e32, 1e-300):.2f}  bound {bound:.2e}")
    assert bound <= LC.CEIL[kind], f"{what}: the fp32 oracle's own error {e32:.3e} puts the bound {bound:.2e} above {LC.CEIL[kind]:.0e}"
    assert e <= bound, f"{what}: error {e:.3e} against fp64 > {bound:.2e} (fp32 oracle: {e32:.3e})"


IMAGE_RUNS = [(1, 1), (2, 1), (8, 1), (32, 1), (2, 3)]


def _rows(b):
    return list(range(b)) if b <= 8 else [0, 1, 17, 31]


@pytest.mark.parametrize("b,depth", IMAGE_RUNS, ids=[f"b{b}_d{d}" for b, d in IMAGE_RUNS])
def test_image_core_every_sample_vs_fp64(hn, b, depth):
    """cfg2 image, N = 50 176: the fp32 rank-D core, its merge, the small-batch plan (b <= 2: one tile per wave, the chain's merge head)
    and the b = 32 plan (8 splits of 6272).  At b = 32 the oracle runs on rows {0, 1, 17, 31} only (samples are independent)."""
    case = LC.image_case(depth)
    ins = LC.fp32_inputs(LC.inputs(case, list(range(b))))
    model = _model(hn, case)
    with torch.no_grad():
        emb = model(_dev(ins), return_embeddings=True).cpu()
        logits = model(_dev(ins)).cpu()
    rows = _rows(b)
    sub = [t[rows] for t in ins]
    for ret, got in (("embeddings", emb[rows]), ("logits", logits[rows])):
        r64 = LC.oracle(case, sub, return_embeddings=ret == "embeddings", device=DEV)
        r32 = LC.oracle(case, sub, return_embeddings=ret == "embeddings", device=DEV, dtype=torch.float32)
        for i, s in enumerate(rows):
            _check(got[i], r64[i], r32[i], "fp32", f"cfg2 d{depth} b={b} sample {s} {ret}")


def _rowwise(a, ref):
    """max over rows of max_t |a - ref| / max_t |ref| (rows = every dim but the last)."""
    a, ref = a.double(), ref.double()
    return float(((a - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)).max())


def test_attention_weights_and_importance_all_tokens(hn):
    """cfg2 b = 2: get_attention_weights() / get_attention_importance() of the image block over ALL 50 176 tokens, elementwise, each row
    against its own maximum (hn_attn_probs / hn_attn_importance rebuild P from the core's statistics)."""
    case = LC.image_case(1)
    ins = LC.fp32_inputs(LC.inputs(case, [0, 1]))
    model = _model(hn, case)
    with torch.no_grad():
        model(_dev(ins))
    w = model.get_attention_weights()[1]
    imp = model.get_attention_importance()[1]
    refs = {}
    for dt in (torch.float64, torch.float32):
        tr = O.FusionTrace()
        sd = {k: v.to(DEV, dt) for k, v in case.sd.items()}
        with torch.device(DEV), torch.no_grad():
            O.fusion_forward(sd, case.cfg(), [t.to(DEV, dt) for t in ins], trace=tr)
        refs[dt] = O.attention_weights_in_module_order(tr, case.cfg())[1]
    p64, p32 = refs[torch.float64], refs[torch.float32]
    assert w.shape == p64.shape and imp.shape == p64.shape[:1] + p64.shape[2:]
    for what, got, r64, r32 in (("weights", w, p64, p32), ("importance", imp, p64.mean(1), p32.mean(1))):
        e, e32 = _rowwise(got, r64), _rowwise(r32, r64)
        bound = max(LC.K * e32, LC.FLOOR["probs"])
        print(f"cfg2 b=2 attention {what}: HIP {e:.3e}  fp32 oracle {e32:.3e}  ratio {e / max(e32, 1e-300):.2f}")
        assert bound <= LC.CEIL["probs"]
        assert e <= bound, f"attention {what}: row-relative error {e:.3e} > {bound:.2e}"


@pytest.mark.parametrize("b", [1, 8])
def test_bag_default_route_vs_fp64(hn, b):
    """cfg4 bag 4096 x 768 (explicit binding): b = 1 runs the fp32-MFMA projection, b = 8 (32 768 rows) the x6 route."""
    case = LC.bag_case()
    ins = LC.fp32_inputs(LC.inputs(case, list(range(b))))
    model = _model(hn, case)
    with torch.no_grad():
        emb = model(_dev(ins), return_embeddings=True).cpu()
    r64 = LC.oracle(case, ins, device=DEV)
    r32 = LC.oracle(case, ins, device=DEV, dtype=torch.float32)
    for i in range(b):
        _check(emb[i], r64[i], r32[i], "fp32", f"cfg4 b={b} sample {i} embeddings")


_ROUTE_SCRIPT = """
import sys, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
import healnet_amd as hn
import long_context_cases as LC
case = LC.bag_case()
model = hn.HealNet(**case.kw).eval()
model.load_state_dict(case.sd)
model = model.to("cuda:0")
out = {{}}
with torch.no_grad():
    for b in (1, 8):
        ins = LC.fp32_inputs(LC.inputs(case, list(range(b))))
        out[b] = model([t.float().to("cuda:0") for t in ins], return_embeddings=True).cpu()
torch.save(out, sys.argv[1])
"""


@pytest.mark.parametrize("route", ["HN_FORCE_X6_GEMM", "HN_NO_X6_GEMM"])
def test_bag_forced_routes_vs_fp64(route, tmp_path):
    """Both patch-bag projection routes at b = 1 and 8, each forced in a fresh process (as test_gpu_x6.py's routes fixture)."""
    script = tmp_path / "run.py"
    script.write_text(_ROUTE_SCRIPT.format(root=ROOT))
    env = {k: v for k, v in os.environ.items() if k not in ("HN_FORCE_X6_GEMM", "HN_NO_X6_GEMM")}
    env[route] = "1"
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "out.pt")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(tmp_path / "out.pt")
    case = LC.bag_case()
    ins = LC.fp32_inputs(LC.inputs(case, list(range(8))))
    r64 = LC.oracle(case, ins, device=DEV)
    r32 = LC.oracle(case, ins, device=DEV, dtype=torch.float32)
    for b in (1, 8):
        for i in range(b):
            _check(got[b][i], r64[i], r32[i], "fp32", f"cfg4 {route} b={b} sample {i} embeddings")


def test_masked_needle_bag_vs_fp64(hn):
    """One 4096-row bag with a key mask (padding rows zero, as bag_padding_mask expects them) and a 1000x needle on a masked row:
    the reference never sees it, so any leak into the softmax is O(1)."""
    case = LC.masked_bag_case()
    ins, mask = LC.masked_inputs(case, [0, 1])
    ins = LC.fp32_inputs(ins)
    model = _model(hn, case)
    with torch.no_grad():
        emb = model(_dev(ins), mask=mask.to(DEV), return_embeddings=True).cpu()
    r64 = LC.oracle(case, ins, mask=mask, device=DEV)
    r32 = LC.oracle(case, ins, mask=mask, device=DEV, dtype=torch.float32)
    for i in range(2):
        _check(emb[i], r64[i], r32[i], "fp32", f"masked bag sample {i} embeddings")


def test_volume_core_every_sample_vs_fp64(hn):
    """cfg3 with the volume cut to 4 frames (N = 200 704), b = 2: the longest token ranges.  The fp64 reference runs the oracle's
    token-chunked softmax."""
    case = LC.volume_case()
    ins = LC.fp32_inputs(LC.inputs(case, [0, 1]))
    model = _model(hn, case)
    with torch.no_grad():
        emb = model(_dev(ins), return_embeddings=True).cpu()
    r64 = LC.oracle(case, ins, device=DEV, token_chunk=1 << 15)
    r32 = LC.oracle(case, ins, device=DEV, dtype=torch.float32, token_chunk=1 << 15)
    for i in range(2):
        _check(emb[i], r64[i], r32[i], "fp32", f"cfg3 volume sample {i} embeddings")


@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_long_context_gradients_vs_fp64(hn, name):
    """Taping forward + fused backward at b = 2: every parameter gradient of the long-context cross blocks (dK/dV of attention_bwd,
    the dQ split reduce, the backward split plan), elementwise against fp64 oracle autograd."""
    case = LC.image_case(1) if name == "cfg2" else LC.bag_case()
    ins = LC.fp32_inputs(LC.inputs(case, [0, 1]))
    dl = torch.linspace(-1.0, 1.5, 2 * case.kw["out_dims"], dtype=torch.float64).reshape(2, -1)
    model = _model(hn, case, train=True)
    y = model(_dev(ins))
    (y * dl.float().to(DEV)).sum().backward()
    g64 = LC.oracle_grads(case, ins, dl, device=DEV)
    g32 = LC.oracle_grads(case, ins, dl, device=DEV, dtype=torch.float32)
    params = dict(model.named_parameters())
    for k in LC.long_block_keys(case):
        _check(params[k].grad, g64[k], g32[k], "grad", f"{name} b=2 grad {k}")


def test_bf16_cores_vs_fp64(hn):
    """core_precision "bf16x3" (documented 1e-3) on the embeddings and "bf16" (documented 2e-2) on the image block's contribution
    (embeddings minus those of the same forward without the image), cfg2 b = 2."""
    case = LC.image_case(1)
    ins = LC.fp32_inputs(LC.inputs(case, [0, 1]))
    r64 = LC.oracle(case, ins, device=DEV)
    r64_skip = LC.oracle(case, [ins[0], None], device=DEV)
    for prec in ("bf16x3", "bf16"):
        model = _model(hn, case, core_precision=prec)
        with torch.no_grad():
            emb = model(_dev(ins), return_embeddings=True).cpu()
            skip = model(_dev([ins[0], None]), return_embeddings=True).cpu()
        for i in range(2):
            if prec == "bf16x3":
                e = LC.err(emb[i], r64[i])
            else:
                e = LC.err(emb[i] - skip[i], r64[i] - r64_skip[i])
            print(f"cfg2 b=2 {prec} sample {i}: {e:.3e} (tolerance {LC.CEIL[prec]:.0e})")
            assert e <= LC.CEIL[prec], f"{prec} sample {i}: {e:.3e} > {LC.CEIL[prec]:.0e}"
