"""The projection shortcut's BatchNorm evaluated inside the bottleneck block's last BatchNorm passes (include/xv2.h "shortcut
fusion") against the unfused launches it replaces, on the same inputs.

Bit-equal: z, its byte mask and the recorded max |z|; dy3 and dy_ds and their recorded maxima; the fp64 sums of both layers and
dgamma / dbeta of both.  The error of dy_ds and of the shortcut's dgamma against the float64 restatement (tests/bn_ref.py) is
printed; the two paths being equal, it is one figure.  Block level: Bottleneck / StBottleneck steps with XV2_SHORTCUT_FUSE = 1
and 0 in two fresh processes (the switch is read at import) must agree bit for bit in output, input gradient, every parameter
gradient and the running statistics, and the profiler must name the fused kernels in one run and in one run only.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import bn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = ("bn_act_shortcut_fwd_kernel", "column_partials_shortcut_kernel", "bn_act_shortcut_bwd_rows_kernel")
RELU, LEAKY = 1, 2

# C = 64: a block covers all channels with 16 lanes; 256: one 256-channel group; 512: two groups along grid.y
# pixels: fewer rows than a chunk's minimum; not a multiple of the rows per pass; several chunks
CASES = [(C, dims) for C in (64, 256, 512) for dims in ((2, 4, 4), (1, 37, 41), (2, 64, 64))]
TWO_PHASE = (256, (2, 136, 128))          # more than 1024 partial rows: reduce_stats takes its two-phase kernel
CASES.append(TWO_PHASE)


def _chunks(npix, C):
    """chunk_geom's rule (csrc/norm_act.hip), vector path: 4 channels per lane for both storage types"""
    groups = C // 256 if (C > 256 and C % 256 == 0) else 1
    rpp = 256 // ((C // groups) // 4)
    rpb = -(-npix * groups // 2048)
    rpb = max(-(-rpb // rpp) * rpp, rpp * 8)
    return -(-npix // rpb)


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(0x55)
    return t


def _coeffs(y, C, g):
    yf = y.float().reshape(-1, C)
    mean = yf.mean(0)
    invstd = 1.0 / torch.sqrt(yf.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.2
    scale = (gamma * invstd).contiguous()
    return dict(mean=mean.contiguous(), invstd=invstd.contiguous(), gamma=gamma, scale=scale,
                shift=(beta - mean * scale).contiguous())


_inputs_memo = {}


def _inputs(C, dims, half):
    """seeded inputs of one case, computed once and shared (never written to)"""
    key = (C, dims, half)
    if key not in _inputs_memo:
        _inputs_memo.clear()              # (one case's tensors at a time)
        N, H, W = dims
        g = torch.Generator(device=DEV).manual_seed(1000 + C + N * H * W)
        dt = torch.bfloat16 if half else torch.float32
        y3 = (torch.randn(N, H, W, C, generator=g, device=DEV) * 1.5 + 0.3).to(dt)
        yd = (torch.randn(N, H, W, C, generator=g, device=DEV) * 0.7 - 0.2).to(dt)
        dz = (torch.randn(N, H, W, C, generator=g, device=DEV) * 0.01).to(dt)
        _inputs_memo[key] = dict(y3=y3, yd=yd, dz=dz, b3=_coeffs(y3, C, g), bd=_coeffs(yd, C, g))
    return _inputs_memo[key]


def _run(t, C, dims, act, fused):
    """forward + backward of the block tail's two BatchNorms through the C ABI, every output poisoned beforehand"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query, set_amax
    N, H, W = dims
    npix = N * H * W
    y3, yd, dz, b3, bd = t["y3"], t["yd"], t["dz"], t["b3"], t["bd"]
    dt = ops._dt(y3)
    z, dy3, dyd = _poison(y3.shape, y3.dtype), _poison(y3.shape, y3.dtype), _poison(y3.shape, y3.dtype)
    zmask = _poison((npix * (C // 4),), torch.uint8)
    dg3, db3, dgd, dbd = (_poison((C,), torch.float32) for _ in range(4))
    az, a3, ad = (torch.zeros(ops.AMAX_BYTES // 4, dtype=torch.int32, device=DEV) for _ in range(3))
    dres = None
    if fused:
        sums2 = _poison((2 * C, 2), torch.float64)
        set_amax(None, None, None, az)
        call("xv2_bn_act_shortcut_forward", y3, yd, b3["scale"], b3["shift"], bd["scale"], bd["shift"], act, z, zmask, npix, C, dt)
        ws = _poison(((query("xv2_bn_act_shortcut_backward_workspace", npix, C) + 3) // 4 + 4,), torch.float32)
        set_amax(None, None, None, a3)
        call("xv2_bn_act_shortcut_backward", dz, zmask, y3, yd, b3["mean"], b3["invstd"], b3["gamma"], bd["mean"], bd["invstd"],
             bd["gamma"], act, float(npix), dy3, dyd, npix, C, sums2, dg3, db3, dgd, dbd, ad, ws, dt)
        s3, sd = sums2[:C], sums2[C:]
    else:
        idt, dres = _poison(y3.shape, y3.dtype), _poison(y3.shape, y3.dtype)
        s3, sd = _poison((C, 2), torch.float64), _poison((C, 2), torch.float64)
        call("xv2_bn_act_forward", yd, C, bd["scale"], bd["shift"], None, 0, ops.ACT_NONE, idt, C, npix, C, dt)
        set_amax(None, None, None, az)
        call("xv2_bn_act_forward_mask", y3, C, b3["scale"], b3["shift"], idt, C, act, z, C, npix, C, zmask, dt)
        ws = _poison(((query("xv2_bn_backward_workspace", npix, C) + 3) // 4 + 4,), torch.float32)
        set_amax(None, None, None, a3)
        call("xv2_bn_act_backward", dz, C, None, C, zmask, y3, C, b3["mean"], b3["invstd"], b3["gamma"], b3["scale"], b3["shift"],
             act, float(npix), dy3, C, dres, C, npix, C, s3, dg3, db3, ws, dt)
        set_amax(None, None, None, ad)
        call("xv2_bn_act_backward", dres, C, None, C, None, yd, C, bd["mean"], bd["invstd"], bd["gamma"], bd["scale"], bd["shift"],
             ops.ACT_NONE, float(npix), dyd, C, None, C, npix, C, sd, dgd, dbd, ws, dt)
    torch.cuda.synchronize()
    return dict(z=z, zmask=zmask, dy3=dy3, dyd=dyd, sums3=s3, sumsd=sd, dgamma3=dg3, dbeta3=db3, dgammad=dgd, dbetad=dbd,
                amax_z=az, amax_dy3=a3, amax_dyd=ad, dres=dres)


KEYS = ("z", "zmask", "dy3", "dyd", "sums3", "sumsd", "dgamma3", "dbeta3", "dgammad", "dbetad")


@pytest.mark.parametrize("act", [RELU, LEAKY], ids=["relu", "leaky"])
@pytest.mark.parametrize("case", CASES, ids=["C%d-%dx%dx%d" % ((c,) + d) for c, d in CASES])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_fused_matches_unfused(half, case, act):
    from xview2_amd._capi import query
    C, dims = case
    npix = dims[0] * dims[1] * dims[2]
    assert query("xv2_bn_act_shortcut_supported", npix, C, 1 if half else 0) == 1
    if case == TWO_PHASE:
        assert _chunks(npix, C) > bn_ref.RS1_MAX_TILES, _chunks(npix, C)
    t = _inputs(C, dims, half)
    u = _run(t, C, dims, act, fused=False)
    f = _run(t, C, dims, act, fused=True)
    bad = [k for k in KEYS if not torch.equal(f[k], u[k])]
    # (a tensor's maximum is the maximum of its 64 slots; which block records into which slot is the pass's own business)
    for k in ("amax_z", "amax_dy3", "amax_dyd"):
        if int(f[k].max()) != int(u[k].max()):
            bad.append(k)
    assert not bad, bad
    for k in ("z", "dy3", "dyd", "sums3", "sumsd", "dgamma3", "dbeta3", "dgammad", "dbetad"):
        assert bool(torch.isfinite(f[k].double()).all()), k
    if half:
        assert all(int(f[k].max()) == 0 for k in ("amax_z", "amax_dy3", "amax_dyd"))      # (fp32 tensors only)
    else:
        for k, v in (("amax_z", f["z"]), ("amax_dy3", f["dy3"]), ("amax_dyd", f["dyd"])):
            assert int(f[k].max()) == bn_ref.amax_bits(v), k
    # the shortcut's dy and dgamma against float64: the residual gradient is the tensor the unfused path stored
    bd = t["bd"]
    yd2, dres2 = t["yd"].reshape(-1, C), u["dres"].reshape(-1, C)
    sums_ref, sbound, parts = bn_ref.backward_sums(dres2, yd2, bd["mean"], bd["invstd"], bn_ref.NONE, pre=dres2)
    dy_ref, dbound, _, _ = bn_ref.backward_apply(parts, f["sumsd"], float(npix), bd["invstd"], bd["gamma"], 1, half)
    e_dy = (f["dyd"].reshape(-1, C).double() - dy_ref).abs()
    e_dg = (f["dgammad"].double() - sums_ref[:, 1]).abs()
    print("C=%d %s %s act=%d: dy_ds max err %.3e (%.3f of its bound), shortcut dgamma max err %.3e (%.3f of its bound)" % (
        C, dims, "bf16" if half else "fp32", act, float(e_dy.max()), float((e_dy / dbound.clamp_min(1e-300)).max()),
        float(e_dg.max()), float((e_dg / bn_ref.f32_of(sums_ref[:, 1], sbound[:, 1]).clamp_min(1e-300)).max())))


def test_fused_is_deterministic():
    C, dims = 512, (1, 37, 41)
    t = _inputs(C, dims, False)
    a = _run(t, C, dims, RELU, fused=True)
    b = _run(t, C, dims, RELU, fused=True)
    for k in KEYS + ("amax_z", "amax_dy3", "amax_dyd"):
        assert torch.equal(a[k], b[k]), k


def test_no_fused_form_without_the_vector_path():
    """C = 96 (24 lanes do not divide 256, no 256-channel groups): `supported` says no and the entry points refuse"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query
    assert query("xv2_bn_act_shortcut_supported", 2 * 32 * 32, 96, 0) == 0
    assert query("xv2_bn_act_shortcut_supported", 2 * 32 * 32, 96, 1) == 0
    y = torch.zeros(2, 4, 4, 96, device=DEV)
    v = torch.zeros(96, device=DEV)
    with pytest.raises(RuntimeError, match="no fused form"):
        call("xv2_bn_act_shortcut_forward", y, y, v, v, v, v, RELU, torch.empty_like(y),
             torch.empty(32 * 24, dtype=torch.uint8, device=DEV), 32, 96, ops.XV2_F32)


# ------------------------------------------------------------------------------------------------ block level
def _blocks():
    """name -> (constructor, input channels, asks for the input alias); inputs are 2 x 32 x 32"""
    from torch import nn
    from xview2_amd import encoders
    from xview2_amd import nn as xnn

    class Tail96(nn.Module):
        """the block tail alone at C = 96, a channel count without a fused form: xnn.bottleneck_tail falls back"""

        def __init__(self):
            super().__init__()
            self.conv3, self.bn3 = nn.Conv2d(32, 96, 1, bias=False), nn.BatchNorm2d(96)
            self.conv_ds, self.bn_ds = nn.Conv2d(64, 96, 1, bias=False), nn.BatchNorm2d(96)
            self.conv1, self.bn1 = nn.Conv2d(64, 32, 1, bias=False), nn.BatchNorm2d(32)

        def forward(self, x):
            out, x = xnn.conv_bn_act(self.conv1, self.bn1, x, act=1, passthrough=True)
            return xnn.bottleneck_tail(self.conv3, self.bn3, out, self.conv_ds, self.bn_ds, x)

    def st(layer):
        return lambda: getattr(encoders.ResNeSt([1, 1, 1, 1], 32), layer)[0]

    return {
        "bottleneck_s1": (lambda: encoders.Bottleneck(64, 64, 1, True), 64, False),
        "bottleneck_s1_alias": (lambda: encoders.Bottleneck(64, 64, 1, True), 64, True),
        "bottleneck_s2": (lambda: encoders.Bottleneck(256, 128, 2, True), 256, False),
        "bottleneck_s2_alias": (lambda: encoders.Bottleneck(256, 128, 2, True), 256, True),
        "resnest_first": (st("layer1"), 64, False),
        "resnest_first_alias": (st("layer1"), 64, True),
        "resnest_s2_alias": (st("layer2"), 256, True),
        "tail96": (Tail96, 64, False),
    }


FALLBACK = ("tail96",)


def _child(out_path):
    """one process: every block, fp32 and bf16 storage, one training step each; results to out_path"""
    from tests.test_f16x2_gpu import _prof
    from xview2_amd import nn as xnn
    res = {}
    for name, (make, cin, alias) in _blocks().items():
        for half in (False, True):
            torch.manual_seed(7)
            blk = make()
            g = torch.Generator().manual_seed(11)
            for m in blk.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
                    m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
            blk = blk.to(DEV).train()
            dt = torch.bfloat16 if half else torch.float32
            x = (torch.randn(2, 32, 32, cin, generator=g) * 0.8).to(DEV).to(dt).requires_grad_(True)
            with _prof() as pr:
                if alias:
                    z, xa = xnn.stage_with_input_alias(blk, x)
                    assert xa is not x
                    wz = torch.randn(z.shape, generator=g).to(DEV)
                    wa = torch.randn(xa.shape, generator=g).to(DEV)
                    ((z.float() * wz).sum() + (xa.float() * wa).sum()).backward()
                else:
                    z = blk(x)
                    wz = torch.randn(z.shape, generator=g).to(DEV)
                    (z.float() * wz).sum().backward()
                names = pr.names()
            key = "%s/%s" % (name, "bf16" if half else "fp32")
            res[key] = dict(z=z.detach().cpu(), dx=x.grad.detach().cpu(), names=names,
                            grads={k: p.grad.detach().cpu() for k, p in blk.named_parameters()},
                            state={k: v.detach().cpu() for k, v in blk.state_dict().items()})
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def block_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("shortcut")
    out = {}
    for fuse in ("1", "0"):
        path = str(d / ("fuse%s.pt" % fuse))
        env = dict(os.environ, XV2_SHORTCUT_FUSE=fuse)
        r = subprocess.run([sys.executable, "-c", "from tests.test_shortcut_fused_gpu import _child; _child(%r)" % path],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        out[fuse] = torch.load(path)
    return out


def test_blocks_match_unfused_bit_for_bit(block_runs):
    f, u = block_runs["1"], block_runs["0"]
    assert set(f) == set(u) and len(f) == 2 * len(_blocks())
    for key in f:
        a, b = f[key], u[key]
        assert torch.equal(a["z"], b["z"]), key
        assert torch.equal(a["dx"], b["dx"]), key
        assert set(a["grads"]) == set(b["grads"]) and set(a["state"]) == set(b["state"])
        for k in a["grads"]:
            assert torch.equal(a["grads"][k], b["grads"][k]), (key, k)
            assert bool(torch.isfinite(a["grads"][k]).all()), (key, k)
        for k in a["state"]:          # running statistics and num_batches_tracked included
            assert torch.equal(a["state"][k], b["state"][k]), (key, k)
        assert any("running_var" in k for k in a["state"])


def test_profiler_names_the_fused_kernels_in_one_run_only(block_runs):
    for key, r in block_runs["0"].items():
        assert not any(n in r["names"] for n in FUSED), (key, r["names"])
    for key, r in block_runs["1"].items():
        if key.split("/")[0] in FALLBACK:
            assert not any(n in r["names"] for n in FUSED), (key, r["names"])
        else:
            assert all(r["names"].count(n) == 1 for n in FUSED), (key, r["names"])
