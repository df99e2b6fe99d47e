"""xBD label files to target PNGs: DATA/labels/*{pre,post}*.json -> DATA/targets/<name>.png, painted on the MI355X.

Pre files paint every building 1; post files paint no-damage 1, minor-damage 2, major-damage 3, destroyed 4 and un-classified
255, in file order with the last building winning.  The fill is utils/rasterize.py's (include/xv2.h states it): under
`--rule reference` the exterior ring with vertices rounded to whole pixels, sampled at the lattice points.  That rule is this
project's own and is NOT pinned to cv2.fillPoly: a fill that also draws the edge lines, as fillPoly and Pillow's
ImageDraw.polygon do, adds pixels up to half a pixel outside slanted edges, so these targets are slightly thinner there;
axis-aligned rectangles agree exactly with Pillow.  `--rule exact` keeps the holes and samples pixel centres in the polygon
rounded to 1/256 pixel.

    python -m xview2_amd.utils.convert2png --data DATA [--n_jobs N] [--batch 16] [--rule reference|exact] [--size 1024]
                                           [--index CSV]
"""
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from concurrent.futures import ThreadPoolExecutor

from . import rasterize

MAX_THREADS = 16


def get_parser():
    p = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, description="Rasterise xBD building polygons into the "
                       "targets/*.png the loaders read.  The fill rule is this project's own, not pinned to cv2.fillPoly: "
                       "targets are slightly thinner along slanted edges than a fill that also draws the edge lines.")
    p.add_argument("--data", type=str, required=True, help="Dataset directory: labels/ is read, targets/ is written")
    p.add_argument("--n_jobs", type=int, default=-1, help="Threads that parse JSON and write PNGs (at most 16; -1: 16)")
    p.add_argument("--batch", type=int, default=16, help="Tiles per device call")
    p.add_argument("--rule", choices=("reference", "exact"), default="reference",
                   help="reference: exterior only, vertices rounded to pixels, lattice samples; exact: holes kept, pixel centres")
    p.add_argument("--size", type=int, default=1024, help="Tile side in pixels")
    p.add_argument("--index", type=str, default=None, metavar="CSV",
                   help="Also write the training index (pytorch_loader.build_index) of DATA to this file")
    return p


parser = get_parser()


def threads_for(n_jobs):
    """the pool size: 1..16; -1 (or anything below 1) selects the 16-thread maximum, never the machine's core count"""
    n_jobs = int(n_jobs)
    return MAX_THREADS if n_jobs < 1 else min(n_jobs, MAX_THREADS)


def label_files(data):
    """[(path, mode)] of DATA/labels in name order: a JSON file whose name holds "post" is painted with damage values, one
    whose name holds "pre" with 1; other files are not label files"""
    folder = os.path.join(data, "labels")
    jobs = []
    for name in sorted(os.listdir(folder)):
        if name.endswith(".json"):
            mode = "post" if "post" in name else "pre" if "pre" in name else None
            if mode:
                jobs.append((os.path.join(folder, name), mode))
    return jobs


class Converter:
    """Converter(args).run(): args needs `data`; n_jobs, batch, rule, size and index default as in get_parser()"""

    def __init__(self, args):
        opt = vars(get_parser().parse_args(["--data", str(args.data)]))
        opt.update({k: v for k, v in vars(args).items() if k in opt})
        self.data, self.rule, self.index = opt["data"], opt["rule"], opt["index"]
        self.size, self.batch, self.threads = int(opt["size"]), max(1, int(opt["batch"])), threads_for(opt["n_jobs"])
        self.jobs = label_files(self.data)

    def run(self):
        """paints every label file; returns how many.  A batch is parsed on the pool, painted in one device call, and its PNGs
        are written on the pool while the next batch is parsed."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("xview2_amd.utils.convert2png runs on the MI355X only; there is no CPU fallback")
        targets = os.path.join(self.data, "targets")
        os.makedirs(targets, exist_ok=True)
        with ThreadPoolExecutor(self.threads) as pool:
            writes = []
            for i in range(0, len(self.jobs), self.batch):
                part = self.jobs[i:i + self.batch]
                tiles = list(pool.map(lambda job: rasterize.read_xbd_json(*job), part))
                maps = rasterize.rasterize(tiles, self.size, self.size, self.rule).cpu().numpy()
                for (path, _), m in zip(part, maps):
                    stem = os.path.splitext(os.path.basename(path))[0]
                    writes.append(pool.submit(rasterize.write_png, os.path.join(targets, stem + ".png"), m))
            for w in writes:
                w.result()
        if self.index:
            from ..data_loading.pytorch_loader import build_index
            build_index(self.data, self.index)
        return len(self.jobs)


def main(argv=None):
    return Converter(get_parser().parse_args(argv)).run()


if __name__ == "__main__":
    print("%d label files" % main())
