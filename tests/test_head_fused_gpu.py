"""The <= 4-channel head of the last decoder layer evaluated inside that layer's BatchNorm passes (include/xv2.h "head fusion")
against the unfused kernels it replaces, on the same inputs.

Bit-equal: logits, dy into the convolution, dgamma / dbeta (and the fp64 sums behind them), the recorded maximum of dy - and the
head's own dw / db: the fused apply pass walks the tensor in head_bwd_kernel's pixel partition (dy is elementwise, so that pass
is free to), which keeps every partial sum of the head's gradients in its place.  Both paths are also measured against a
float64 restatement of dw / db (the exact sum of the same fp32 terms: dlogits x the stored z); the figures are printed.
"""
import copy

import pytest
import torch

from tests.golden.cases import ARGS, MODEL_CASES, labels, model_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED = ("bn_act_head_fwd_kernel", "column_partials_kernel<head>", "bn_act_bwd_rows_head_kernel")
UNFUSED = ("head_fwd_kernel", "head_bwd_kernel")

SHAPES = {"64x64": (2, 64, 64), "odd": (1, 37, 41), "full": (2, 1024, 1024)}
C = 32


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(0x55)
    return t


def _inputs(shape, cout, nchw, half, seed):
    N, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt = torch.bfloat16 if half else torch.float32
    y = (torch.randn(N, H, W, C, generator=g, device=DEV) * 1.5 + 0.3).to(dt)
    yf = y.float().reshape(-1, C)
    mean = yf.mean(0)
    invstd = 1.0 / torch.sqrt(yf.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.2
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    w = (torch.randn(cout, C, generator=g, device=DEV) * 0.2).contiguous()
    b = torch.randn(cout, generator=g, device=DEV)
    dl = torch.randn((N, cout, H, W) if nchw else (N, H, W, cout), generator=g, device=DEV) * 0.01
    return dict(y=y, mean=mean.contiguous(), invstd=invstd.contiguous(), gamma=gamma, scale=scale, shift=shift, w=w, b=b, dl=dl)


def _run(t, shape, cout, nchw, fused):
    """forward + backward of BatchNorm apply + LeakyReLU + head through the C ABI, every output poisoned beforehand"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query, set_amax
    N, H, W = shape
    npix, hw = N * H * W, H * W
    y = t["y"]
    dt = ops._dt(y)
    act = ops.ACT_LEAKY
    logits = _poison((N, cout, H, W) if nchw else (N, H, W, cout), torch.float32)
    dy = _poison(y.shape, y.dtype)
    dw, db = _poison((cout, C), torch.float32), _poison((cout,), torch.float32)
    dgamma, dbeta = _poison((C,), torch.float32), _poison((C,), torch.float32)
    sums2 = _poison((C, 2), torch.float64)
    slots = torch.zeros(ops.AMAX_BYTES // 4, dtype=torch.int32, device=DEV)
    z = None
    if fused:
        call("xv2_bn_act_head_forward", y, C, t["scale"], t["shift"], act, npix, hw, C, cout, t["w"], t["b"], logits,
             1 if nchw else 0, dt)
        ws = _poison(((query("xv2_bn_act_head_backward_workspace", npix, C, cout) + 3) // 4 + 4,), torch.float32)
        set_amax(None, None, None, slots)
        call("xv2_bn_act_head_backward", t["dl"], 1 if nchw else 0, hw, t["w"], cout, y, C, t["mean"], t["invstd"], t["gamma"],
             t["scale"], t["shift"], act, float(npix), dy, C, npix, C, sums2, dgamma, dbeta, dw, db, ws, dt)
    else:
        z = _poison(y.shape, y.dtype)
        dz = _poison(y.shape, y.dtype)
        call("xv2_bn_act_forward", y, C, t["scale"], t["shift"], None, 0, act, z, C, npix, C, dt)
        call("xv2_head_conv_forward", z, C, npix, hw, C, cout, t["w"], t["b"], logits, 1 if nchw else 0, dt)
        ws = _poison(((query("xv2_head_conv_backward_workspace", npix, C, cout) + 3) // 4 + 4,), torch.float32)
        call("xv2_head_conv_backward", z, C, t["dl"], npix, hw, C, cout, t["w"], 1 if nchw else 0, dz, C, dw, db, ws, dt)
        ws2 = _poison(((query("xv2_bn_backward_workspace", npix, C) + 3) // 4 + 4,), torch.float32)
        set_amax(None, None, None, slots)
        call("xv2_bn_act_backward", dz, C, None, C, None, y, C, t["mean"], t["invstd"], t["gamma"], t["scale"], t["shift"], act,
             float(npix), dy, C, None, C, npix, C, sums2, dgamma, dbeta, ws2, dt)
        del dz
    torch.cuda.synchronize()
    return dict(logits=logits, dy=dy, dw=dw, db=db, dgamma=dgamma, dbeta=dbeta, sums2=sums2, amax=slots, z=z)


def _head_grad_ref(z, dl, cout, nchw):
    """float64 restatement of the head's dw / db: the exact sums of the fp32 terms both paths add"""
    g = (dl.permute(0, 2, 3, 1) if nchw else dl).reshape(-1, cout).double()
    dw = torch.zeros(cout, C, dtype=torch.float64, device=DEV)
    zf = z.reshape(-1, C)
    step = 1 << 18
    for s in range(0, zf.shape[0], step):          # (chunks: the fp64 copy of the full-size z would be half a gigabyte)
        dw += g[s:s + step].t() @ zf[s:s + step].double()
    return dw, g.sum(0)


def _gate(name, fused, unfused, ref):
    e_f = float((fused.double() - ref).abs().max())
    e_u = float((unfused.double() - ref).abs().max())
    floor = float(ref.abs().max()) * 2.0 ** -23
    print("%s: fused err %.3e unfused err %.3e (ratio %.2f) floor %.3e" % (name, e_f, e_u, e_f / max(e_u, 1e-300), floor))
    assert e_f == e_u, (name, e_f, e_u)
    return e_f / max(e_u, floor)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("nchw", [True, False], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_fused_matches_unfused(half, cout, nchw, shape):
    from xview2_amd._capi import query
    dims = SHAPES[shape]
    assert query("xv2_bn_act_head_supported", dims[0] * dims[1] * dims[2], C, cout) == 1
    worst = 0.0
    for seed in ((3,) if shape == "full" else (3, 4, 5)):
        t = _inputs(dims, cout, nchw, half, seed)
        u = _run(t, dims, cout, nchw, fused=False)
        f = _run(t, dims, cout, nchw, fused=True)
        bad = [k for k in ("logits", "sums2", "dgamma", "dbeta", "dy", "dw", "db") if not torch.equal(f[k], u[k])]
        # (the maximum of dy is the maximum of its 64 slots; which block records into which slot is the pass's own business)
        if int(f["amax"].max()) != int(u["amax"].max()):
            bad.append("amax")
        assert not bad, (bad, seed)
        assert bool(torch.isfinite(f["dw"]).all()) and bool(torch.isfinite(f["db"]).all())
        if not half:
            assert int(u["amax"].max()) > 0          # the maximum of dy was recorded (fp32 tensors) - and equals the fused one
        dw_ref, db_ref = _head_grad_ref(u["z"], t["dl"], cout, nchw)
        worst = max(worst, _gate("dw %s seed %d" % (shape, seed), f["dw"], u["dw"], dw_ref),
                    _gate("db %s seed %d" % (shape, seed), f["db"], u["db"], db_ref))
        del t, u, f
    print("worst fused / max(unfused, floor) ratio: %.2f" % worst)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_fused_is_deterministic(half):
    dims = SHAPES["odd"]
    t = _inputs(dims, 2, True, half, 9)
    a = _run(t, dims, 2, True, fused=True)
    b = _run(t, dims, 2, True, fused=True)
    for k in ("logits", "dy", "dw", "db", "dgamma", "dbeta", "sums2", "amax"):
        assert torch.equal(a[k], b[k]), k
    dims = SHAPES["64x64"]
    t = _inputs(dims, 4, False, half, 10)
    a = _run(t, dims, 4, False, fused=True)
    b = _run(t, dims, 4, False, fused=True)
    for k in ("logits", "dy", "dw", "db", "dgamma", "dbeta", "sums2", "amax"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ whole model
def _model(a, seed=1):
    from xview2_amd import networks
    from xview2_amd.weights import deterministic_init_
    torch.manual_seed(0)
    m = networks.UNetLoc(a) if a.type == "pre" else networks.get_dmg_unet(a)
    deterministic_init_(m, seed)
    return m.to(DEV)


class _head_fuse:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from xview2_amd import ops
        self.old, ops.HEAD_FUSE = ops.HEAD_FUSE, self.on

    def __exit__(self, *exc):
        from xview2_amd import ops
        ops.HEAD_FUSE = self.old


def _step(model, a, x, y):
    from xview2_amd import criterion
    model.train()
    keep = {}
    pred = model(x)
    p0 = pred[0] if isinstance(pred, list) else pred
    p0.register_hook(lambda g: keep.__setitem__("dlogits", g.detach().clone()))
    loss = criterion.compute_loss(criterion.Loss(a), pred, y, a.deep_supervision)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), p0.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}, keep["dlogits"]


def test_model_step_matches_unfused():
    from tests.test_f16x2_gpu import _prof
    a = ARGS(**MODEL_CASES["pre_resnet50"])
    x, y = model_input(a).to(DEV), labels(a).to(DEV)
    m0 = _model(a)
    m_u, m_f, m_z = copy.deepcopy(m0), copy.deepcopy(m0), copy.deepcopy(m0)
    with _head_fuse(False), _prof() as pr:
        loss_u, log_u, g_u, dl = _step(m_u, a, x, y)
        names_u = pr.names()
    with _head_fuse(True), _prof() as pr:
        loss_f, log_f, g_f, _ = _step(m_f, a, x, y)
        names_f = pr.names()
    assert all(n in names_f for n in FUSED) and not any(n in names_f for n in UNFUSED), names_f
    assert all(n in names_u for n in UNFUSED) and not any(n in names_u for n in FUSED), names_u
    assert torch.equal(loss_f, loss_u) and torch.equal(log_f, log_u)
    head = ("output_block.output_block.conv.weight", "output_block.output_block.conv.bias")
    assert set(g_f) == set(g_u) and all(h in g_f for h in head)
    for k in g_u:
        assert torch.equal(g_f[k], g_u[k]), k
    # the head's gradients against the exact sums: z = what the decoder hands the head when the blocks run on their own
    from xview2_amd import nn as xnn
    m_z.train()
    with torch.no_grad():
        z = m_z.unet(xnn.to_nhwc_image(x))[0]
    dw_ref, db_ref = _head_grad_ref(z, dl, dl.shape[1], True)
    _gate("model dw", g_f[head[0]].reshape(dw_ref.shape), g_u[head[0]].reshape(dw_ref.shape), dw_ref)
    _gate("model db", g_f[head[1]], g_u[head[1]], db_ref)


def _names_of_step(a, train=True, split=False):
    from tests.test_f16x2_gpu import _prof
    from xview2_amd import nn as xnn
    m = _model(a)
    x, y = model_input(a).to(DEV), labels(a).to(DEV)
    with _prof() as pr:
        if not train:
            m.eval()
            with torch.no_grad():
                m(x)
        elif split:
            m.train()
            with xnn.bn_split(2):
                p = m(x)
            p.float().sum().backward()
        else:
            _step(m, a, x, y)
        return pr.names()


def test_unfused_kernels_keep_their_cases():
    """the Siamese concat of two dec5, deep-supervision heads, an active bn_split and eval mode run the kernels they ran before"""
    # Siamese: the head reads the concat of the pre and the post pass (and the passes run under bn_split)
    n = _names_of_step(ARGS(**MODEL_CASES["post_siamese_coral"]))
    assert n.count("head_fwd_kernel") == 1 and n.count("head_bwd_kernel") == 1 and not any(k in n for k in FUSED), n
    # deep supervision: the heads on dec4 / dec3 stay head kernels; the main head on dec5 is the fused one
    n = _names_of_step(ARGS(**dict(MODEL_CASES["pre_resnet50"], deep_supervision=True)))
    assert n.count("head_fwd_kernel") == 2 and n.count("head_bwd_kernel") == 2 and all(n.count(k) == 1 for k in FUSED), n
    # an active bn_split
    n = _names_of_step(ARGS(**MODEL_CASES["pre_resnet50"]), split=True)
    assert n.count("head_fwd_kernel") == 1 and n.count("head_bwd_kernel") == 1 and not any(k in n for k in FUSED), n
    # eval
    n = _names_of_step(ARGS(**MODEL_CASES["pre_resnet50"]), train=False)
    assert n.count("head_fwd_kernel") == 1 and not any(k in n for k in FUSED), n


def test_a_watched_decoder_keeps_its_output():
    """a forward hook on the last decoder level is a second consumer of dec5: the level returns its features, the head runs unfused"""
    from tests.test_f16x2_gpu import _prof
    a = ARGS(**MODEL_CASES["pre_resnet50"])
    m = _model(a)
    x, y = model_input(a).to(DEV), labels(a).to(DEV)
    got = []
    h = m.unet.dec_l5.register_forward_hook(lambda mod, inp, out: got.append(tuple(out.shape)))
    try:
        with _prof() as pr:
            _step(m, a, x, y)
            n = pr.names()
    finally:
        h.remove()
    assert got == [(2, 64, 64, 32)], got
    assert n.count("head_fwd_kernel") == 1 and n.count("head_bwd_kernel") == 1 and not any(k in n for k in FUSED), n
    with _prof() as pr:          # hook gone: fused again
        _step(m, a, x, y)
        n = pr.names()
    assert all(n.count(k) == 1 for k in FUSED) and not any(k in n for k in UNFUSED), n
    m.train()
    with torch.no_grad():        # no gradients: nothing to save, the blocks return what they always returned
        from xview2_amd import nn as xnn
        assert tuple(m.unet(xnn.to_nhwc_image(x))[0].shape) == (2, 64, 64, 32)


def test_blocks_on_their_own_return_features():
    """ConvBlock / UpsampleBlock called as modules keep returning the activated features (the block-wise parity tests rely on it)"""
    from xview2_amd.decoder import ConvBlock
    blk = ConvBlock(32, 32).to(DEV).train()
    x = torch.randn(2, 16, 16, 32, device=DEV)
    out = blk(x)
    assert tuple(out.shape) == (2, 16, 16, 32)
    head = torch.nn.Conv2d(32, 2, kernel_size=1).to(DEV)
    logits = copy.deepcopy(blk)(x, head=head)
    assert tuple(logits.shape) == (2, 2, 16, 16)
    from xview2_amd import nn as xnn
    assert torch.equal(logits, xnn.head_conv(head, copy.deepcopy(blk)(x)))
