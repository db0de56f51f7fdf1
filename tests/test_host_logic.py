"""CPU: host-side logic of the drop-in package (no compute): constructor / state_dict / RNG-order
parity with the reference, error behaviour, and the C-ABI library's exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT
from healnet_amd import Attention, HealNet, MMDataset, _capi
from oracle import healnet_cpu as O


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "healnet_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(hn_[a-z_0-9]+)\s*\(", header, flags=re.M))
    assert declared == set(_capi.SIGNATURES), declared ^ set(_capi.SIGNATURES)
    lib = _capi.lib()                      # raises if the .so is missing: build() must have run
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.hn_abi_version() == _capi.HN_ABI_VERSION == 12
    assert lib.hn_context_pitch(13, 64) == 16 and lib.hn_context_pitch(18, 64) == 32
    assert lib.hn_context_pitch(773, 64) == 776 and lib.hn_context_pitch(2005, 64) == 2008
    assert lib.hn_context_pitch(20, 16) == 20          # rank-D path would not pay: dp 32 > dim_head 16


def test_error_codes_without_gpu():
    lib = _capi.lib()
    p = _capi.AttnParams(heads=8, dim_head=200, query_dim=128)
    assert lib.hn_attn_workspace_bytes(ctypes.byref(p), 1, 16, 2, 128, 100, 13) == 0
    assert b"dim_head" in lib.hn_last_error_string()
    p = _capi.AttnParams(heads=8, dim_head=64, query_dim=128)
    need = lib.hn_attn_workspace_bytes(ctypes.byref(p), 1, 16, 32, 128, 50176, 13)
    assert 0 < need < 200 << 20
    f = _capi.FFParams(dim=128, gate=0)
    assert lib.hn_ff_workspace_bytes(ctypes.byref(f), 4096) == 4096 * 640 * 4      # hidden (rows, 4 dim) + the pre-dropout output (rows, dim)
    # NULL pointers are reported, not dereferenced
    rc = lib.hn_head_fwd(None, 1, 1, 1, None, None, None, None, 1, None, None)
    assert rc == -5


def test_constructor_assertions_match_reference():
    with pytest.raises(AssertionError):
        HealNet(n_modalities=1, channel_dims=[2189, 100], num_spatial_axes=[1, 1], out_dims=4)   # tests/test_healnet.py:63-67
    with pytest.raises(AssertionError):
        HealNet(n_modalities=2, channel_dims=[3], num_spatial_axes=[1], out_dims=4)


def _key_sums(model):
    sd = model.state_dict()
    keys = sorted(sd.keys())
    return keys, np.array([float(sd[k].double().sum()) for k in keys]), np.array([float(sd[k].double().abs().sum()) for k in keys])


def test_seeded_init_is_bit_compatible_with_reference(manifest):
    """Same RNG consumption order as the reference constructor (a1): identical per-key checksums."""
    g = load_golden("kat0")
    torch.manual_seed(0)
    model = HealNet(**manifest["kat0"]["kwargs"])
    keys, sums, abssums = _key_sums(model)
    assert keys == manifest["kat0"]["state_keys"]
    assert len(keys) == 125 and sum(p.numel() for p in model.parameters()) == 9587024
    np.testing.assert_allclose(sums, g["key_sums"].numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(abssums, g["key_abssums"].numpy(), rtol=0, atol=1e-9)
    assert torch.allclose(model.latents[0, :3], torch.tensor([-1.12583983, -1.15236020, -0.25057858]))


@pytest.mark.parametrize("tag", ["tied", "m3", "noself"])
def test_init_variants_keys_and_tying(tag, manifest):
    m = manifest["kat_init_" + tag]
    g = load_golden("kat_init_" + tag)
    torch.manual_seed(5)
    model = HealNet(**m["kwargs"])
    keys, sums, abssums = _key_sums(model)
    assert keys == m["state_keys"]
    np.testing.assert_allclose(sums, g["key_sums"].numpy(), atol=1e-9)
    np.testing.assert_allclose(abssums, g["key_abssums"].numpy(), atol=1e-9)
    assert sum(p.numel() for p in model.parameters()) == m["n_params"]
    sd = model.state_dict()
    groups = {}
    for k in keys:
        groups.setdefault(sd[k].data_ptr(), []).append(k)
    mine = sorted(sorted(v) for v in groups.values() if len(v) > 1)
    assert mine == sorted(sorted(v) for v in m["shared_groups"])


def test_state_dict_roundtrip_with_oracle_layout():
    kw = dict(n_modalities=2, channel_dims=[20, 3], num_spatial_axes=[1, 2], out_dims=3, l_c=8, l_d=16, x_heads=2,
              l_heads=2, cross_dim_head=4, latent_dim_head=4)
    model = HealNet(**kw)
    shapes = O.state_dict_shapes(O.FusionConfig(**kw))
    sd = model.state_dict()
    assert set(sd) == set(shapes)
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == tuple(s), k
    model.load_state_dict(O.filler_state_dict(O.FusionConfig(**kw)), strict=True)


def test_cpu_tensors_are_rejected_loudly():
    model = HealNet(n_modalities=1, channel_dims=[4], num_spatial_axes=[1], out_dims=2, l_c=4, l_d=8, x_heads=1,
                    l_heads=1, cross_dim_head=4, latent_dim_head=4).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model([torch.rand(2, 3, 4)])
    att = Attention(8, 5, heads=2, dim_head=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        att(torch.rand(1, 3, 8), context=torch.rand(1, 4, 5))


def test_unsupported_modes_raise():
    # the stand-alone modules drop in training mode like the reference's nn.Dropout (round 6: the rate and a per-call (seed, offset,
    # stream) triple go to the kernels; tests/test_gpu_dropout.py) -- on the CPU box: a triple is drawn in training mode only
    from healnet_amd.healnet import _draw_rng
    att = Attention(8, 5, heads=2, dim_head=4, dropout=0.1).train()
    p, rng = _draw_rng(att, 0)
    assert p == pytest.approx(0.1) and len(rng) == 3 and rng[1] == 1 and att._last_rng == tuple(rng)
    assert _draw_rng(att, 0)[1][1] == 2                       # a fresh offset (fresh masks) per call
    assert _draw_rng(att.eval(), 0) == (0.0, [])
    m = HealNet(n_modalities=1, channel_dims=[4], num_spatial_axes=[1], out_dims=2, l_c=4, l_d=8, x_heads=1, l_heads=1,
                cross_dim_head=4, latent_dim_head=4, attn_dropout=0.1)
    assert m.train()._dropout_active() and not m.eval()._dropout_active()
    m2 = HealNet(n_modalities=1, channel_dims=[4], num_spatial_axes=[1], out_dims=2, l_c=4, l_d=8, x_heads=1, l_heads=1,
                 cross_dim_head=4, latent_dim_head=4, self_per_cross_attn=2).eval()
    with pytest.raises(ValueError):
        m2([torch.rand(2, 3, 4)])


def test_mmdataset_semantics():
    a, b_ = torch.arange(6).reshape(3, 2), torch.arange(12).reshape(3, 4)
    ds = MMDataset([a, b_])
    assert len(ds) == 3 and torch.equal(ds[1][0], a[1]) and torch.equal(ds[1][1], b_[1])
    ds2 = MMDataset([a, b_], target=torch.tensor([7, 8, 9]))
    sample, y = ds2[2]
    assert int(y) == 9 and torch.equal(sample[1], b_[2])


def test_module_level_names_of_the_reference_exist():
    """from healnet.models.healnet import ... keeps working after the import swap (healnet.py module surface)."""
    import healnet_amd as h
    for name in ["HealNet", "Attention", "PreNorm", "FeedForward", "GELU", "SELU", "fourier_encode", "temperature_softmax", "cache_fn",
                 "exists", "default"]:
        assert hasattr(h, name), name
    assert h.exists(0) and not h.exists(None) and h.default(None, 3) == 3 and h.default(2, 3) == 2
    calls = []
    f = h.cache_fn(lambda: calls.append(1) or len(calls))
    assert f(key="a") == 1 and f(key="a") == 1 and f(key="b") == 2 and f(_cache=False) == 3 and f(key="a") == 1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU fallback: without libhealnet_hip.so every product entry point raises (the oracle is never consulted)."""
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", str(tmp_path / "libhealnet_hip.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _capi.lib()
    import sys
    assert not any(name.startswith("oracle") for name in sys.modules if "healnet_amd" in (getattr(sys.modules[name], "__file__", "") or "")), \
        "the product package must not import the oracle"
    import healnet_amd
    import healnet_amd.dist, healnet_amd.etl, healnet_amd.ops, healnet_amd.train      # noqa: F401
    src = "".join(open(getattr(m, "__file__")).read() for m in (healnet_amd, healnet_amd.healnet, healnet_amd.train, healnet_amd.etl,
                                                                healnet_amd.dist, healnet_amd.ops, healnet_amd._capi))
    assert "import oracle" not in src and "from oracle" not in src


def test_standalone_blocks_refuse_a_context_that_requires_grad():
    """The stand-alone Attention is differentiable w.r.t. x and its parameters (torch.ops.healnet_hip.attention_fwd + the
    registered backward); NO gradient flows to the context (hn_attn_bwd), so a context that requires grad must raise rather
    than silently train nothing -- checked before any device work, so it runs on the CPU."""
    import healnet_amd as hn
    with pytest.raises(RuntimeError, match="no gradient flows to the context"):
        hn.PreNorm(16, hn.Attention(16, 5, heads=2, dim_head=8), context_dim=5)(torch.randn(2, 4, 16), context=torch.randn(2, 3, 5, requires_grad=True))
    with pytest.raises(RuntimeError, match="no gradient flows to the context"):
        hn.Attention(16, 5, heads=2, dim_head=8)(torch.randn(2, 4, 16), context=torch.randn(2, 3, 5, requires_grad=True))


def test_operator_schemas_and_fake_kernels():
    """torch.ops.healnet_hip.* is the route of the package: every operator is registered, has a fake (meta) kernel for
    tracing, and the fusion operators' fake kernels size their outputs from the C library's own planning functions."""
    import healnet_amd as hn
    ops = torch.ops.healnet_hip
    for name in ["fusion_forward", "fusion_forward_train", "fusion_backward", "attention", "attention_fwd", "attention_bwd",
                 "feed_forward", "feed_forward_bwd", "head", "head_bwd", "fourier_encode_concat", "encode_norm", "temperature_softmax"]:
        assert hasattr(ops, name), name
    from torch._subclasses.fake_tensor import FakeTensorMode
    model = hn.HealNet(n_modalities=2, channel_dims=[7, 3], num_spatial_axes=[1, 2], out_dims=3, depth=2, l_c=8, l_d=16, x_heads=2,
                       l_heads=2, cross_dim_head=8, latent_dim_head=8)
    spec = model._spec_text
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        params = [mode.from_tensor(p.detach()) for p in model.parameters()]
        tab, img = mode.from_tensor(torch.rand(5, 1, 7)), mode.from_tensor(torch.rand(5, 6, 4, 3))
        out, stats, trace = ops.fusion_forward([tab, img], None, params, spec, 0, False, True)
        assert out.shape == (5, 3) and trace.shape == (2 * 3, 5, 8, 16) and stats.shape == (6, 5 * 2 * 8 * 2)
        out, tape, layout = ops.fusion_forward_train([tab, None], None, params, spec, 0, True, None, None, [])
        assert out.shape == (5, 8, 16) and tape.dtype == torch.uint8 and tape.numel() > 0 and layout.shape == (12,)
        y, st, saved = ops.attention_fwd(mode.from_tensor(torch.rand(2, 8, 16)), None, None, None, None, None, None, params[4], params[5],
                                         params[6], params[7], 2, True, True)
        assert y.shape == (2, 8, 16) and st.shape == (2, 2, 8, 2) and saved.numel() > 0


def test_fused_adam_state_is_checkpointed():
    """the Adam moments and the update count live in Optimizer.state, so state_dict() / load_state_dict() resume them
    (structure only here -- the arithmetic is covered by the GPU fixtures)."""
    import healnet_amd as hn

    class _Flat:          # FlatParameters without a device
        def __init__(self):
            self.params = torch.zeros(8)
            self.grads = torch.zeros(8)
            self.views = [torch.nn.Parameter(self.params[:8].view(2, 4))]
            self.offsets = [0]
            self.numel = 8
    import unittest.mock as mock
    with mock.patch.object(hn.train._capi, "lib") as lib:
        lib.return_value.hn_l1_adam_workspace_bytes.return_value = 256
        opt = hn.train.FusedL1Adam(_Flat(), lr=1e-3)
        opt.state[opt.flat.views[0]]["step"] = 7
        opt.exp_avg.fill_(0.5)
        sd = opt.state_dict()
        assert sd["state"][0]["step"] == 7 and float(sd["state"][0]["exp_avg"].sum()) == 4.0
        opt2 = hn.train.FusedL1Adam(_Flat(), lr=1e-3)
        opt2.load_state_dict(sd)
        assert opt2._steps == 7 and float(opt2.exp_avg.sum()) == 4.0 and opt2.exp_avg.shape == (8,)


def _cpu_flat(shapes, outside=()):
    """A FlatParameters laid out on the host (the class refuses host tensors; its layout logic does not need a device)."""
    import healnet_amd as hn
    f = hn.train.FlatParameters.__new__(hn.train.FlatParameters)
    sizes = [(int(torch.tensor(s).prod()) + 3) // 4 * 4 for s in shapes]
    f.numel = sum(sizes)
    f.params, f.grads = torch.zeros(f.numel), torch.zeros(f.numel)
    f.views, f.offsets, f.outside = [], [], list(outside)
    off = 0
    for s, n in zip(shapes, sizes):
        k = int(torch.tensor(s).prod())
        p = torch.nn.Parameter(f.params[off:off + k].view(s))
        p.grad = f.grads[off:off + k].view(s)
        f.views.append(p)
        f.offsets.append(off)
        off += n
    return f


def test_fused_adam_launch_plan_with_frozen_parameters():
    """one hn_l1_adam_step over the whole buffer per step while every view is trainable; with a view frozen
    after flattening, one launch per run of trainable views (16-byte aligned starts, the frozen slot never swept), reg_loss from a
    separate reduction (the launches get NULL), and per-view update counts so a view that sat out resumes with its own count;
    a parameter frozen before flattening counts in reg_loss and unfreezing it raises."""
    import unittest.mock as mock
    import healnet_amd as hn
    frozen_out = torch.nn.Parameter(torch.full((3,), -2.0), requires_grad=False)
    f = _cpu_flat([(2, 3), (5,), (4,), (3, 3)], outside=[frozen_out])
    f.params.copy_(torch.arange(f.numel, dtype=torch.float32) - 10)
    with mock.patch.object(hn.train._capi, "lib") as lib, mock.patch.object(hn.train, "_stream", return_value=0):
        lib.return_value.hn_l1_adam_workspace_bytes.return_value = 256
        lib.return_value.hn_l1_adam_step.return_value = 0
        call = lib.return_value.hn_l1_adam_step
        opt = hn.train.FusedL1Adam(f, lr=1e-3, l1=0.5)
        base = f.params.data_ptr()

        def launches():
            out = [((c.args[0] - base) // 4, c.args[4], c.args[11], c.args[12]) for c in call.call_args_list]
            call.reset_mock()
            return out
        for step in (1, 2):
            opt.step()
            got = launches()
            assert len(got) == 1 and got[0][:3] == (0, f.numel, step) and got[0][3] == opt.reg_loss.data_ptr()
        assert "view_skips" not in opt.state[f.views[0]]
        f.views[1].requires_grad_(False)                      # frozen after flattening: slot [8, 16)
        for step in (3, 4):
            opt.step()
            assert launches() == [(0, 8, step, None), (16, 16, step, None)]
            assert float(opt.reg_loss) == pytest.approx(0.5 * (float(f.params.abs().sum()) + 6.0))
        f.views[1].requires_grad_(True)                       # resumes with its own count (2 updates so far, this is its 3rd)
        opt.step()
        assert launches() == [(0, 8, 5, None), (8, 8, 3, None), (16, 16, 5, None)]
        assert opt.state[f.views[0]]["view_skips"] == [0, 2, 0, 0]
        assert all(f.offsets[i] % 4 == 0 for i in range(4))
        frozen_out.requires_grad_(True)                       # frozen before flattening, unfrozen since: it has no slot
        with pytest.raises(RuntimeError, match="flatten_parameters"):
            opt.step()
        assert not call.called


def test_non_fp32_parameters_are_refused():
    """model.half() / .bfloat16() / .double() would make the kernels read the wrong bytes: the descriptor refuses."""
    model = HealNet(n_modalities=1, channel_dims=[3], num_spatial_axes=[2], out_dims=2, depth=1, l_c=4, l_d=8, x_heads=1,
                    l_heads=1, cross_dim_head=8, latent_dim_head=8)
    model._descriptor()                                   # fp32: fine (pointer marshalling only, no device needed)
    for cast in ("bfloat16", "half", "double"):
        with pytest.raises(TypeError, match="float32"):
            getattr(HealNet(n_modalities=1, channel_dims=[3], num_spatial_axes=[2], out_dims=2, depth=1, l_c=4, l_d=8, x_heads=1,
                            l_heads=1, cross_dim_head=8, latent_dim_head=8), cast)()._descriptor()


def test_reference_import_lines_resolve():
    """The import lines a user of konst-int-i/healnet writes (README.md:70-71, healnet/models/__init__.py:1-11, main.py, explainer.py,
    tests/test_healnet.py) resolve to the HIP-backed classes -- executed verbatim."""
    ns = {}
    exec("from healnet import HealNet\n"
         "from healnet.etl import MMDataset\n"
         "from healnet.models import HealNet as H2, Attention\n"
         "from healnet.models import *\n"
         "from healnet.models.healnet import fourier_encode, temperature_softmax, Attention as A2\n"
         "from healnet.etl.loaders import MMDataset as M2\n", ns)
    import healnet_amd
    assert ns["HealNet"] is ns["H2"] is healnet_amd.HealNet
    assert ns["Attention"] is ns["A2"] is healnet_amd.Attention
    assert ns["MMDataset"] is ns["M2"] is healnet_amd.MMDataset
    assert ns["fourier_encode"] is healnet_amd.fourier_encode
    import healnet.models as hm
    with pytest.raises(AttributeError, match="not provided"):
        hm.FCNN  # noqa: B018  (out of scope: named, not silently missing)


def test_build_id_is_content_addressed(tmp_path):
    """The library embeds the digest of the sources + flags it was built from; the host side trusts a prebuilt copy exactly when
    that digest matches the sources next to it (never by mtime)."""
    from healnet_amd import _capi
    lib = _capi.lib()
    want = _capi.source_build_id()
    assert lib.hn_build_id().decode() == want == _capi.library_build_id()
    assert len(want) == 16 and int(want, 16) >= 0
    # the digest moves with the flags and with any source byte
    hipcc, flags = _capi._flags()
    a = _capi._digest(_capi._headers(), " ".join([hipcc] + flags))
    b = _capi._digest(_capi._headers(), " ".join([hipcc] + flags + ["-DX"]))
    assert a != b
    p = tmp_path / "x.h"
    p.write_text("int a;")
    d1 = _capi._digest([str(p)], "f")
    p.write_text("int b;")
    assert _capi._digest([str(p)], "f") != d1
    # a file without the marker (or a missing one) has no id
    q = tmp_path / "lib.so"
    q.write_bytes(b"\x7fELF" + b"\0" * 64)
    assert _capi.library_build_id(str(q)) is None and _capi.library_build_id(str(tmp_path / "none.so")) is None


def test_parameter_slots_follow_reregistration():
    """HealNet._params() caches (module, name) slots; replacing a submodule or adding a parameter after the first use must be
    seen: the list stays identical to list(parameters())."""
    import healnet_amd
    from torch import nn
    m = healnet_amd.HealNet(n_modalities=1, channel_dims=[8], num_spatial_axes=[1], out_dims=2, depth=1, l_c=4, l_d=8, x_heads=1,
                            l_heads=1, cross_dim_head=4, latent_dim_head=4)
    ids = lambda ps: [id(p) for p in ps]      # noqa: E731
    assert ids(m._params()) == ids(m.parameters())
    m.to_logits[2] = nn.Linear(8, 2)
    assert ids(m._params()) == ids(m.parameters())
    m.extra = nn.Parameter(torch.zeros(3))
    assert ids(m._params()) == ids(m.parameters())


def test_descriptor_cache_key_sees_dtype_and_layout():
    from healnet_amd import ops
    a, b = torch.zeros(4, 4), torch.zeros(4, 4)
    k0 = ops.Spec._param_key([a, b])
    assert k0 == ops.Spec._param_key([a, b])
    assert ops.Spec._param_key([a, b.t()]) != k0 or b.t().is_contiguous()
    c = torch.zeros(4, 4, dtype=torch.float64)
    assert ops.Spec._param_key([a, c])[2][1] is False


def test_four_processes_against_a_stale_library_cpu(tmp_path):
    """N ranks starting on a box whose library does not match its sources (VERDICT r4 weak 1 / ADVICE r4): one relinks under the
    build lock, all load the fresh file.  The same body runs on the GPU box from tests/test_gpu_cluster.py."""
    from test_gpu_cluster import run_stale_library_race
    run_stale_library_race(tmp_path, procs=4)
