"""Cost of matching predicted to labelled buildings (csrc/match.hip) next to the two xv2_building_table calls on the same
maps, and next to the host restatement.

    timeout -k 10 900 python scripts/bench_match.py [--iters 50] [--rounds 3] [--out profiles/match_cost.md]

One process.  Four shapes: B = 1, 8 and 32 tiles of 1024 x 1024 with about 300 rectangular buildings each and a prediction
that moves every edge by up to 3 pixels and leaves one building in eight out (tests/match_ref.town), and one 4096 x 4096
scene of the same generator.  Capacities are the modules' first capacities.  Per shape, event-timed after warm-up, the legs
alternating within every round:
  match   the launches of xv2_building_match on preallocated buffers (labels, tables and workspace resident)
  tables  the two xv2_building_table calls (prediction and target) that produce its inputs from resident labels
Then once per shape the launch-bracketing profiler's time per kernel of one match call, the module call
utils.building_metrics.match_maps (labelling, tables, match and the copies to the host) by the host clock, and the host
restatement tests/match_ref.match of tile 0.  The GPU match of tile 0 is compared with the restatement at the timed sizes.
Writes the record as markdown to --out and prints it.  Not a test; it gates nothing."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import buildings_ref as BR  # noqa: E402
import match_ref as MR  # noqa: E402
from bench_buildings import kernel_times, timed  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import building_metrics, buildings  # noqa: E402


def maps(n, H, W):
    """uint8 [n,H,W] x 4: pre / post of the prediction, pre / post of the target"""
    out = [[], [], [], []]
    for k in range(n):
        pre_t, pre_p = MR.town(700 + k, H, W), MR.town(700 + k, H, W, jitter=800 + k)
        cls = np.kron(BR._hash(900 + k, (H // 64, W // 64), 4) + 1, np.ones((64, 64), dtype=np.int64)).astype(np.uint8)
        flip = np.where(BR._hash(950 + k, (H, W), 8) == 0, np.uint8(5) - cls, cls)
        for lst, a in zip(out, (pre_p, flip * pre_p, pre_t, cls * pre_t)):
            lst.append(a.astype(np.uint8))
    return [np.stack(x) for x in out]


def bench_shape(name, host_maps, iters, rounds, lines):
    dev = torch.device("cuda", 0)
    pre_p, post_p, pre_t, post_t = (torch.from_numpy(m).to(dev) for m in host_maps)
    B, H, W = pre_p.shape
    cap_rows = buildings.first_capacity(H, W)
    lab_p, lab_t = ops.label_components(pre_p), ops.label_components(pre_t)
    rows_p, count_p = ops.building_table(lab_p, post_p, None, cap_rows)
    rows_t, count_t = ops.building_table(lab_t, post_t, None, cap_rows)
    assert int(count_p.max()) <= cap_rows and int(count_t.max()) <= cap_rows
    cap = building_metrics.first_capacity(H, W)
    need = int(_capi.query("xv2_building_match_workspace", B, H, W, cap))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tws = torch.empty(int(_capi.query("xv2_building_table_workspace", B, H, W)), dtype=torch.uint8, device=dev)
    match_p = torch.empty((B, cap_rows, 8), dtype=torch.int64, device=dev)
    match_t = torch.empty((B, cap_rows, 8), dtype=torch.int64, device=dev)
    pieces = torch.empty((B,), dtype=torch.int32, device=dev)

    def run_match():
        _capi.call("xv2_building_match", lab_p, rows_p, count_p, cap_rows, lab_t, rows_t, count_t, cap_rows, B, H, W, 1, 2, cap,
                   ws, match_p, match_t, pieces)

    def run_tables():
        _capi.call("xv2_building_table", lab_p, post_p, None, B, H, W, cap_rows, tws, rows_p, count_p)
        _capi.call("xv2_building_table", lab_t, post_t, None, B, H, W, cap_rows, tws, rows_t, count_t)

    legs = {"match": run_match, "tables": run_tables}
    for fn in legs.values():                     # warm-up of every leg at this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    n_pieces = pieces.cpu().numpy()
    assert int(n_pieces.max()) <= cap, "first capacity %d below the piece count %d" % (cap, int(n_pieces.max()))
    ks = kernel_times(run_match)
    building_metrics.match_maps(pre_p, post_p, pre_t, post_t)      # the first call of a shape pays torch's allocations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = building_metrics.match_maps(pre_p, post_p, pre_t, post_t)
    t_module = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = MR.match(*(m[0] for m in host_maps))
    t_host = time.perf_counter() - t0
    equal = np.array_equal(got[0].match_p, want["match_p"]) and np.array_equal(got[0].match_t, want["match_t"])
    px = B * H * W
    lines.append("## %s: B = %d, %d x %d" % (name, B, H, W))
    lines.append("")
    show = lambda v: ", ".join(str(int(x)) for x in v[:8]) + (", ..." if len(v) > 8 else "")
    lines.append("Predicted buildings per tile: %s; labelled: %s; overlap pieces: %s (capacity %d rows and %d pieces per tile); "
                 "matched at 1/2 in tile 0: %d." % (show(count_p.cpu().numpy()), show(count_t.cpu().numpy()), show(n_pieces),
                                                   cap_rows, cap, int(want["match_p"][:, 3].sum())))
    lines.append("")
    lines.append("| leg | µs per call, %d rounds of %d calls | median | ns per pixel |" % (rounds, iters))
    lines.append("|---|---|---|---|")
    for k in legs:
        med = statistics.median(times[k])
        lines.append("| %s | %s | %.1f | %.4f |" % (k, ", ".join("%.1f" % t for t in times[k]), med, 1e3 * med / px))
    lines.append("")
    lines.append("Match launches over the two table calls: %.2f." % (statistics.median(times["match"])
                                                                   / statistics.median(times["tables"])))
    lines.append("")
    lines.append("Per kernel, one bracketed match call (the brackets' events add their own overhead): "
                 + ", ".join("`%s` %.1f µs" % kv for kv in sorted(ks.items())) + ".")
    lines.append("")
    lines.append("`utils.building_metrics.match_maps` (labelling, both tables, match, everything copied back), host clock, the "
                 "second call: %.2f ms for the batch.  Host restatement (tests/match_ref.match: labels, both tables, match) of "
                 "tile 0: %.1f ms.  GPU match of tile 0 equal to it: %s." % (1e3 * t_module, 1e3 * t_host, equal))
    lines.append("")
    return equal


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_match.py measures on the MI355X; there is no CPU fallback")
    lines = ["# Cost of matching predicted to labelled buildings (`utils/building_metrics.py`)", "",
             "One MI355X (%s), `python scripts/bench_match.py --iters %d --rounds %d`, one process.  Device events around %d "
             "calls after warm-up, the legs alternating within each round.  Recorded, not gated: nothing calls the match unless "
             "the object-level score is asked for." % (torch.cuda.get_device_name(0), a.iters, a.rounds, a.iters), ""]
    ok = True
    tiles = maps(32, 1024, 1024)
    for B in (1, 8, 32):
        ok = bench_shape("tiles", [m[:B] for m in tiles], a.iters, a.rounds, lines) and ok
    ok = bench_shape("scene", maps(1, 4096, 4096), a.iters, a.rounds, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU match differs from the restatement")


if __name__ == "__main__":
    main()
