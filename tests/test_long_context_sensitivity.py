"""CPU self-check of tests/test_gpu_long_context.py: in fp64 on the host, every corruption a buggy attention core would make (a skipped
end or first tile of each split, a per-sample stride slip, a leaking masked token) moves the oracle's output by at least SENSITIVITY x
the bound the GPU test allows -- so each GPU case fails on the bug class it targets.  Plus the pins of the oracle's token-chunked path
and of the split-plan restatement the needles are placed by."""
import pytest
import torch

import long_context_cases as LC
from oracle import healnet_cpu as O


def _shift(case, ins, samples, kind, b, mask=None):
    """Shift of the LAST sample's embeddings under the mutation (only that sample and, for a stride slip, sample 0 are built)."""
    mi, mm = LC.mutate(case, ins, samples, kind, b, mask)
    last = lambda ts: [None if t is None else t[-1:] for t in ts]
    ref = LC.oracle(case, last(ins), mask=None if mask is None else mask[-1:], token_chunk=1 << 14)
    got = LC.oracle(case, last(mi), mask=None if mm is None else mm[-1:], token_chunk=1 << 14)
    return LC.err(got, ref), ref, got


def _require(shift, tol, what):
    print(f"{what}: reference shift {shift:.3e} ({shift / tol:.0f} x the bound {tol:.0e})")
    assert shift >= LC.SENSITIVITY * tol, f"{what}: the mutation moves the reference by {shift:.3e} < {LC.SENSITIVITY} x {tol:.0e}"


IMAGE = [(1, 1), (2, 1), (8, 1), (32, 1), (2, 3)]


@pytest.mark.parametrize("b,depth", IMAGE, ids=[f"b{b}_d{d}" for b, d in IMAGE])
def test_image_cases_see_every_mutation(b, depth):
    case = LC.image_case(depth)
    rows = list(range(b)) if b <= 8 else [0, 1, 17, 31]
    samples = [rows[0], rows[-1]] if b > 1 else [0]
    ins = LC.fp32_inputs(LC.inputs(case, samples))
    kinds = ["range_ends", "range_starts"] + (["stride"] if b > 1 else [])
    for kind in kinds:
        s, _, _ = _shift(case, ins, samples, kind, b)
        _require(s, LC.CEIL["fp32"], f"cfg2 d{depth} b={b} {kind}")


def test_bf16_case_sees_the_mutations():
    """bf16x3 is checked on the embeddings at 1e-3, bf16 on the image block's contribution at 2e-2 (test_bf16_cores_vs_fp64)."""
    case = LC.image_case(1)
    samples = [0, 1]
    ins = LC.fp32_inputs(LC.inputs(case, samples))
    skip = LC.oracle(case, [ins[0][1:], None])
    for kind in ("range_ends", "stride"):
        s, ref, got = _shift(case, ins, samples, kind, 2)
        _require(s, LC.CEIL["bf16x3"], f"bf16x3 {kind}")
        if kind == "stride":
            # the image block's contribution: a whole foreign context moves it by O(0.1) -- 5x the bf16 tolerance, not 20x; the
            # narrower bug classes are held by the fp32 and bf16x3 cases, which share the token loop and the merge
            sd = LC.err(got - skip, ref - skip)
            print(f"bf16 stride: contribution shift {sd:.3e}")
            assert sd >= 5 * LC.CEIL["bf16"]


def test_attention_weights_case_sees_a_skipped_tile():
    case = LC.image_case(1)
    ins = LC.fp32_inputs(LC.inputs(case, [1]))
    mi, _ = LC.mutate(case, ins, [1], "range_ends", 2)
    ps = []
    for x in (ins, mi):
        tr = O.FusionTrace()
        with torch.no_grad():
            O.fusion_forward(case.sd64(), case.cfg(), x, trace=tr)
        ps.append(O.attention_weights_in_module_order(tr, case.cfg())[1])
    rowwise = lambda a, r: float(((a - r).abs().amax(-1) / r.abs().amax(-1)).max())
    _require(rowwise(ps[1], ps[0]), LC.CEIL["probs"], "attention weights range_ends")
    _require(rowwise(ps[1].mean(1), ps[0].mean(1)), LC.CEIL["probs"], "attention importance range_ends")


@pytest.mark.parametrize("b", [1, 8])
def test_bag_cases_see_every_mutation(b):
    case = LC.bag_case()
    samples = [0, b - 1] if b > 1 else [0]
    ins = LC.fp32_inputs(LC.inputs(case, samples))
    for kind in ["range_ends", "range_starts"] + (["stride"] if b > 1 else []):
        s, _, _ = _shift(case, ins, samples, kind, b)
        _require(s, LC.CEIL["fp32"], f"cfg4 b={b} {kind}")


def test_masked_bag_case_sees_a_leak():
    case = LC.masked_bag_case()
    ins, mask = LC.masked_inputs(case, [0, 1])
    ins = LC.fp32_inputs(ins)
    s, _, _ = _shift(case, ins, [0, 1], "unmask", 2, mask)
    _require(s, LC.CEIL["fp32"], "masked bag unmask")
    s, _, _ = _shift(case, ins, [0, 1], "range_ends", 2, mask)
    _require(s, LC.CEIL["fp32"], "masked bag range_ends")


def test_volume_case_sees_a_skipped_tile():
    case = LC.volume_case()
    ins = LC.fp32_inputs(LC.inputs(case, [0, 1]))
    for kind in ("range_ends", "stride"):
        s, _, _ = _shift(case, ins, [0, 1], kind, 2)
        _require(s, LC.CEIL["fp32"], f"cfg3 volume {kind}")


@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_gradient_cases_see_a_skipped_backward_tile(name):
    case = LC.image_case(1) if name == "cfg2" else LC.bag_case()
    ins = LC.fp32_inputs(LC.inputs(case, [0, 1]))
    dl = torch.linspace(-1.0, 1.5, 2 * case.kw["out_dims"], dtype=torch.float64).reshape(2, -1)
    mi, _ = LC.mutate(case, ins, [0, 1], "bwd_range_ends", 2)
    g = LC.oracle_grads(case, [t[1:] for t in ins], dl[1:])
    gm = LC.oracle_grads(case, [t[1:] for t in mi], dl[1:])
    worst = max(LC.err(gm[k], g[k]) for k in g if "norm" not in k)
    _require(worst, LC.CEIL["grad"], f"{name} gradients bwd_range_ends (largest over the block's weights)")
    least = min(LC.err(gm[k], g[k]) for k in g if "to_kv" in k or "to_q" in k)
    _require(least, LC.CEIL["grad"], f"{name} to_q / to_kv gradients bwd_range_ends")


def test_chunked_oracle_matches_unchunked():
    """The optional token-chunked softmax of oracle.healnet_cpu.attention equals the unchunked path to 1e-12 in fp64, masked rows,
    a ragged last chunk and a chunk that is entirely masked included."""
    g = torch.Generator().manual_seed(3)
    b, L, n, dq, D, heads, e = 2, 20, 301, 24, 13, 4, 8
    x = torch.randn(b, L, dq, generator=g, dtype=torch.float64)
    ctx = torch.randn(b, n, D, generator=g, dtype=torch.float64) * 3
    wq = torch.randn(heads * e, dq, generator=g, dtype=torch.float64) * 2
    wkv = torch.randn(2 * heads * e, D, generator=g, dtype=torch.float64)
    wo = torch.randn(dq, heads * e, generator=g, dtype=torch.float64) * 0.2
    bo = torch.randn(dq, generator=g, dtype=torch.float64)
    mask = torch.rand(b, n, generator=g) > 0.3
    mask[1, 64:128] = False
    for m in (None, mask):
        ref = O.attention(x, ctx, wq, wkv, wo, bo, heads, mask=m)
        for chunk in (1, 64, 100, 301, 1000):
            got = O.attention(x, ctx, wq, wkv, wo, bo, heads, mask=m, token_chunk=chunk)
            assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-12, (chunk, m is not None)


def test_split_plan_restatement():
    """The plans the needles target (attn_core_geometry with the default knobs): cfg2 b = 32 cuts the image into 8 splits of 6272
    tokens, b = 2 runs the small-batch plan (32 splits of 1568); every chunk is a multiple of 16 and the splits cover N."""
    N = 224 * 224
    assert LC.split_plans(32, N, 13)["fwd"] == 6272
    assert LC.split_plans(2, N, 13)["fwd"] == 1568
    for b in (1, 2, 3, 8, 32):
        for D in (13, 18, 773):
            for c in LC.split_plans(b, N, D).values():
                assert c % 16 == 0 and LC._cdiv(N, c) * c >= N > (LC._cdiv(N, c) - 1) * c
