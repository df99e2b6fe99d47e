"""profiles/pmc_traffic.json from two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE; separate runs as the MI355X guide
prescribes).  HBM bytes per launch = (2*FETCH_SIZE + WRITE_SIZE) * 1024: FETCH_SIZE/WRITE_SIZE are in KiB and on gfx950
FETCH_SIZE counts 128-byte requests as 64 bytes for wide coalesced streams (guide, section HBM); WRITE_SIZE is
uncalibrated.  usage: pmc_traffic.py <fetch.db> <write.db> <out.json>"""
import json
import re
import sqlite3
import sys
from collections import defaultdict


def per_kernel(db, counter):
    c = sqlite3.connect(db)
    q = ("select s.kernel_name, e.value, d.id from rocpd_pmc_event e join rocpd_info_pmc p on e.pmc_id = p.id "
         "join rocpd_kernel_dispatch d on e.event_id = d.event_id join rocpd_info_kernel_symbol s on d.kernel_id = s.id "
         "where p.name = '%s'" % counter)
    tot, n = defaultdict(float), defaultdict(set)
    for kn, v, did in c.execute(q):
        tot[kn] += v
        n[kn].add(did)
    return {k: tot[k] / len(n[k]) for k in tot}, {k: len(n[k]) for k in tot}


def pretty(mangled):
    """mangled kernel symbol -> the name bench.py's in-library profiler registers (roofline.kernel)"""
    m = re.match(r"_ZN3xv2\d+wgrad_alltaps(64)?_x3_kernelILi(\d)E", mangled)
    if m:
        return "wgrad_alltaps%s_kernel<%s>" % (m.group(1) or "", "f16x2" if m.group(2) == "2" else "f32x3")
    if "wgrad_alltaps64_tr_kernel" in mangled:
        return "wgrad_alltaps64_kernel<bf16hbm>"
    m = re.match(r"_ZN3xv2\d+wgrad_tr_x3_kernelILi(\d+)ELi(\d+)ELi(\d)E", mangled)
    if m:
        return "wgrad_tr_kernel<%s,%s,%s>" % (m.group(1), m.group(2), "f16x2" if m.group(3) == "2" else "f32x3")
    if "wgrad_alltaps_tr_kernel" in mangled:
        return "wgrad_alltaps_kernel<bf16hbm>"
    if "wgrad_alltaps_kernel" in mangled:
        return "wgrad_alltaps_kernel<bf16>" if "ILb1E" in mangled else "wgrad_alltaps_kernel"
    if "direct3x3_n32_kernel" in mangled:
        if "ILb1ELb1E" in mangled:
            return "direct3x3_n32_kernel<bf16hbm>"
        return "direct3x3_n32_kernel<bf16>" if "ILb1E" in mangled else "direct3x3_n32_kernel"
    m = re.match(r"_ZN3xv2\d+thin1x1_kernelILi(\d+)ELi(\d+)ELb(\d)E", mangled)
    if m:
        return "thin1x1_kernel<%s,%s,%s>" % (m.group(1), m.group(2), "bf16hbm" if m.group(3) == "1" else "f32x3")
    m = re.match(r"_ZN3xv2\d+wgrad_tr_kernelILi(\d+)ELi(\d+)E", mangled)
    if m:
        return "wgrad_tr_kernel<%s,%s,bf16hbm>" % (m.group(1), m.group(2))
    m = re.match(r"_ZN3xv2\d+sg_conv_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)E", mangled)
    if m:
        wm, g, nb, plain, hs = (int(v) for v in m.groups())
        return "sg_conv_kernel<%d,%d,g%d,%s%s>" % (32 * wm, 32 * nb, g, "1x1," if plain else "", "bf16hbm" if hs else "f16x2")
    for nm in ("bn_act_bwd_rows_kernel", "column_partials_kernel", "bn_act_fwd_kernel", "reduce_stats_kernel", "wgrad_reduce_t_kernel",
               "wgrad_reduce_kernel", "splitk_reduce_kernel", "adamw_dev_kernel", "stem7x7_kernel", "stem7x7_wgrad_kernel"):
        if nm in mangled:
            return nm
    m = re.match(r"_ZN3xv2\d+igemm_kernelILNS_4FormE(\d+)ELi(\d+)ELi(\d+)EEEv", mangled)
    if m:      # enum Form of igemm_kernel.h, in its order -> the suffix of FORM_TRAITS there
        form, bm, bn = (int(v) for v in m.groups())
        tag = ("rgb", "rgb,bf16out", "c32", "c32,bf16", "c32,bf16hbm", "c32,bf16hbm,halo", "c32,f32x3", "c32,f32x3,halo",
               "c32,f32x3,halo,wx3", "c32,f16x2", "c32,f16x2,halo,wx2")[form]
        return "igemm_kernel<%d,%d,%d,%d,%s>" % (bm, bn, 4 if bn == 32 else 2, 1 if bn == 32 else 2, tag)
    m = re.match(r"_ZN3xv2\d+wgrad_kernelILNS_5WFormE(\d+)ELi(\d+)ELi(\d+)EEEv", mangled)
    if not m:
        return None      # enum WForm of wgrad_kernel.h, in its order; waves of a block (co x ci x pixels) from the tile as tile_wgm / tile_wk there
    form, bm, bn = (int(v) for v in m.groups())
    tag = ("rgb", "rgb,bf16hbm", "c32", "c32,bf16", "c32,bf16,bf16hbm", "c32,bf16hbm")[form]
    wgm, wgn = min(bm // 32, 2), min(bn // 32, 2)
    return "wgrad_kernel<%d,%d,%d,%d,%d,%s>" % (bm, bn, wgm, wgn, 4 // (wgm * wgn), tag)


f, nf = per_kernel(sys.argv[1], "FETCH_SIZE")
w, _ = per_kernel(sys.argv[2], "WRITE_SIZE")
import os
out = {"_meta": {"commit": os.environ.get("XV2_COMMIT", "unknown"),
                 "note": "tree the PMC passes were taken on (XV2_COMMIT, set by the caller of scripts/profile_bench.sh)"}}
for k in f:
    name = pretty(k)
    if name:
        out[name] = {"fetch_size_kib": round(f[k], 1), "write_size_kib": round(w.get(k, 0.0), 1),
                     "hbm_bytes_per_launch": round((2 * f[k] + w.get(k, 0.0)) * 1024), "launches": nf[k]}
json.dump(out, open(sys.argv[3], "w"), indent=1)
print(json.dumps(out, indent=1))
