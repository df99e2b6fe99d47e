"""Post-processing and xView2 scoring on the MI355X (csrc/postproc.hip): bit-equal to the digests recorded from the
reference's scripts (tests/golden/postproc_golden.json) and to the numpy restatement (tests/postproc_ref.py), batched,
deterministic, the connected-component label contract, and the eval -> post-process -> score flow through the CLIs."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import postproc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "postproc_golden.json")))
VARIANTS = [(c, r) for c in (False, True) for r in (0, 1, 3, 5)]


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()


def _first_diffs(got, want, what):
    ys, xs = np.nonzero(got != want)
    pts = ", ".join("(%d,%d): %d != %d" % (y, x, got[y, x], want[y, x]) for y, x in zip(ys[:8], xs[:8]))
    return "%s: %d pixels differ, first %s" % (what, len(ys), pts)


def _run(loc, dmg, comp, rate):
    from xview2_amd.utils.post_process import post_process_tiles
    pre, post = post_process_tiles(torch.from_numpy(loc).to(DEV), torch.from_numpy(np.ascontiguousarray(dmg)).to(DEV),
                                   components=comp, dilate=rate > 0, dilation_rate=rate or 3)
    return pre.cpu().numpy(), post.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    return R.cases()


@pytest.mark.parametrize("name", sorted(GOLD["postprocess"]))
def test_post_process_tiles_bit_equal(cases, name):
    loc, dmg = cases[name]
    rec = GOLD["postprocess"][name]
    for comp, rate in VARIANTS:
        if comp and name in R.WIDE:   # surviving labels above 4: the vote keeps four classes and refuses them
            with pytest.raises(ValueError, match="outside 1..4"):
                _run(loc, dmg, comp, rate)
            continue
        pre, post = _run(loc, dmg, comp, rate)
        key = "c%d_r%d" % (comp, rate)
        if key in rec and (_digest(pre), _digest(post)) == tuple(rec[key]):
            continue
        rpre, rpost = R.post_process(loc, dmg, comp, rate)
        assert np.array_equal(pre, rpre), _first_diffs(pre, rpre, "%s %s pre" % (name, key))
        assert np.array_equal(post, rpost), _first_diffs(post, rpost, "%s %s post" % (name, key))
        assert key not in rec, "%s %s: equal to the restatement but not to the reference digest" % (name, key)


@pytest.mark.parametrize("name", sorted(R.odd_cases()))
def test_odd_sizes_equal_restatement(name):
    loc, dmg = R.odd_cases()[name]
    for comp, rate in VARIANTS:
        pre, post = _run(loc, dmg, comp, rate)
        rpre, rpost = R.post_process(loc, dmg, comp, rate)
        assert np.array_equal(pre, rpre), _first_diffs(pre, rpre, "%s c%d r%d pre" % (name, comp, rate))
        assert np.array_equal(post, rpost), _first_diffs(post, rpost, "%s c%d r%d post" % (name, comp, rate))


def test_mixed_batch_equals_single_tiles(cases):
    from xview2_amd.utils.post_process import post_process_tiles
    names = ["buildings_4ch", "thresholds", "vote_ties", "mask_spiral", "mask_checkerboard", "mask_percolation"]
    loc = torch.from_numpy(np.stack([cases[n][0] for n in names])).to(DEV)
    dmg = torch.from_numpy(np.stack([cases[n][1] for n in names])).to(DEV)
    pre, post = post_process_tiles(loc, dmg, components=True, dilate=True, dilation_rate=3)
    for i in range(len(names)):
        p1, q1 = post_process_tiles(loc[i], dmg[i], components=True, dilate=True, dilation_rate=3)
        assert torch.equal(pre[i], p1) and torch.equal(post[i], q1), names[i]


def test_runs_are_deterministic(cases):
    loc, dmg = cases["mask_percolation"]
    a = _run(loc, dmg, True, 3)
    b = _run(loc, dmg, True, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("shape", [(1024, 1024), (1000, 777), (65, 3)])
def test_connected_components_label_contract(shape):
    from xview2_amd.utils.post_process import connected_components
    masks = R.adversarial_masks(*shape)
    names = sorted(masks)
    got = connected_components(torch.from_numpy(np.stack([masks[n] for n in names])).to(DEV)).cpu().numpy()
    for i, n in enumerate(names):
        want = R.label_min_index(masks[n])
        assert np.array_equal(got[i], want), _first_diffs(got[i], want, n)
        assert np.array_equal(R.scipy_numbering(got[i]), R.scipy_numbering(want))
    again = connected_components(torch.from_numpy(masks["spiral"]).to(DEV)).cpu().numpy()
    assert np.array_equal(again, got[names.index("spiral")])


def test_five_channel_and_rate_checks():
    from xview2_amd.utils.post_process import post_process_tiles
    loc = torch.full((1, 64, 64), 0.5, device=DEV)
    with pytest.raises(ValueError):
        post_process_tiles(loc, torch.zeros(1, 4, 64, 64, device=DEV), dilate=True, dilation_rate=2)
    five = torch.full((1, 64, 64), 5, dtype=torch.int64, device=DEV)
    assert int(post_process_tiles(loc, five)[1].max()) == 5            # kept, as the reference keeps it
    assert int(post_process_tiles(loc, five, dilate=True)[1].max()) == 5
    with pytest.raises(ValueError, match="outside 1..4"):
        post_process_tiles(loc, five, components=True)
    with pytest.raises(ValueError, match="outside 0..255"):
        post_process_tiles(loc, torch.full((1, 64, 64), 300, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="outside"):
        post_process_tiles(loc, torch.full((1, 64, 64), -2, dtype=torch.int64, device=DEV), components=True)
    # dropped by the fusion (loc <= 0.1): never checked
    low = torch.full((1, 64, 64), 0.05, device=DEV)
    assert int(post_process_tiles(low, five + 100, components=True, dilate=True)[1].max()) == 0
    from xview2_amd import ops
    ws = ops.postprocess_workspace(1, 64, 64, True, DEV)
    with pytest.raises(ValueError, match="workspace"):
        ops.postprocess(loc, torch.zeros(1, 4, 64, 64, device=DEV), components=True, workspace=ws[:100])
    with pytest.raises(ValueError, match="workspace"):
        ops.postprocess(loc, torch.zeros(1, 4, 64, 64, device=DEV), components=True, workspace=ws[16:])
    d5 = torch.rand(1, 5, 64, 64, device=DEV)
    assert torch.equal(post_process_tiles(loc, d5)[1], post_process_tiles(loc, d5[:, 1:5].contiguous())[1])


def _write_tiles(tmp, tiles):
    from PIL import Image
    pred, targ = os.path.join(tmp, "predictions"), os.path.join(tmp, "targets")
    os.makedirs(pred)
    os.makedirs(targ)
    for k, (lp, dp, lt, dt) in enumerate(tiles):
        for d, kind, suffix, a in ((pred, "localization", "prediction", lp), (pred, "damage", "prediction", dp),
                                   (targ, "localization", "target", lt), (targ, "damage", "target", dt)):
            Image.fromarray(a).save(os.path.join(d, "test_%s_%05d_%s.png" % (kind, k, suffix)))
    return pred, targ


def test_score_rows_and_metrics_json(tmp_path):
    from xview2_amd.utils import xview2_metrics as xm
    tiles = R.metric_tiles()
    maps = [torch.from_numpy(np.stack([t[k] for t in tiles])).to(DEV) for k in range(4)]
    rows = xm.score_tiles(*maps)
    assert rows.tolist() == GOLD["metrics"]["rows"]
    pred, targ = _write_tiles(str(tmp_path), tiles)
    out = str(tmp_path / "metrics.json")
    xm.compute_score(pred, targ, out)
    assert open(out).read() == GOLD["metrics"]["json"]
    m = xm.XviewMetrics(pred, targ)
    assert m.score == GOLD["metrics"]["dict"]["score"] and "Harmonic mean" in repr(m)
    bad = maps[1].clone()
    bad[2, 5, 7] = 5
    with pytest.raises(ValueError, match="0-4"):
        xm.score_tiles(maps[0], bad, maps[2], maps[3])


def test_kernels_are_named_by_the_profiler(cases):
    from tests.test_f16x2_gpu import _prof
    from xview2_amd.utils import xview2_metrics as xm
    loc, dmg = cases["buildings_5ch"]
    with _prof() as pr:
        pre, post = _run(loc, dmg, True, 3)
        xm.score_tiles(*[torch.from_numpy(a[None]).to(DEV) for a in (pre, post, pre, post)])
        names = pr.names()
    for k in ("pp_fuse_kernel", "pp_merge_kernel", "pp_compress_kernel", "pp_vote_kernel", "xview2_counts_kernel"):
        assert k in names, names


def _child(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r


def test_eval_post_process_score_end_to_end(tmp_path):
    import main as cli
    res = str(tmp_path / "results")
    common = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
              "--val_batch_size", "2", "--train_size", "64", "--eval_size", "1024", "--steps_per_epoch", "1"]
    cks = {}
    for task, extra in (("pre", ["--loss_str", "dice"]), ("post", ["--loss_str", "dice", "--dmg_model", "siamese"])):
        tr = str(tmp_path / ("train_" + task))
        cli.main(["--exec_mode", "train", "--type", task, "--epochs", "1", "--results", tr] + extra + common)
        cks[task] = os.path.join(tr, "checkpoints", "last.ckpt")
        cli.main(["--exec_mode", "eval", "--type", task, "--ckpt", cks[task], "--results", res] + extra + common)
    probs = sorted(os.listdir(os.path.join(res, "probs")))
    dmg0 = np.load(os.path.join(res, "probs", [p for p in probs if "damage" in p][0]))
    assert dmg0.shape == (4, 1024, 1024), dmg0.shape   # softmax over the four damage classes (networks.get_nclass)
    _child(["-m", "xview2_amd.utils.post_process", "--results", res, "--components", "--dilate", "--batch", "3"], 300)
    out = os.path.join(res, "metrics.json")
    _child(["-m", "xview2_amd.utils.xview2_metrics", os.path.join(res, "predictions"), os.path.join(res, "targets"),
            out], 300)
    from PIL import Image
    rows = []
    locs = sorted(p for p in probs if "localization" in p)
    dmgs = sorted(p for p in probs if "damage" in p)
    assert len(locs) == len(dmgs) > 0
    for a, b in zip(locs, dmgs):
        pre, post = R.post_process(np.load(os.path.join(res, "probs", a)), np.load(os.path.join(res, "probs", b)),
                                   components=True, rate=3)
        gp = np.array(Image.open(os.path.join(res, "predictions", a.replace(".npy", "_prediction.png"))))
        gq = np.array(Image.open(os.path.join(res, "predictions", b.replace(".npy", "_prediction.png"))))
        assert np.array_equal(gp, pre), _first_diffs(gp, pre, a)
        assert np.array_equal(gq, post), _first_diffs(gq, post, b)
        lt = np.array(Image.open(os.path.join(res, "targets", a.replace(".npy", "_target.png"))))
        dt = np.array(Image.open(os.path.join(res, "targets", b.replace(".npy", "_target.png"))))
        rows.append(R.tile_row(pre, post, lt, dt))
    got = json.load(open(out))
    assert got == R.score(rows)
    assert set(got) == {"score", "damage_f1", "localization_f1", "damage_f1_no_damage", "damage_f1_minor_damage",
                        "damage_f1_major_damage", "damage_f1_destroyed"}
