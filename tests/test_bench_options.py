"""bench.py's options (CPU only): what a plain run leaves to --full, and the fixed sample
--dump-outputs takes of every cube."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_checks_and_side_passes_need_full():
    """The oracle check and the PCIe-inclusive pass are --full's: asked for without it, the
    run stops at the command line (before any device work) instead of quietly leaving them out."""
    for extra, msg in ((["--check", "full"], b"--check needs --full"),
                       (["--e2e-size", "300"], b"--e2e-size needs --full"),
                       (["--gpus", "2", "--dump-outputs", "out"], b"--dump-outputs needs --gpus 1")):
        r = _run("--steps", "1", "--warmup", "0", *extra)
        assert r.returncode == 2 and msg in r.stderr, (extra, r.stderr)
        assert not r.stdout.strip()


def test_dump_sample_is_fixed_and_inside_the_cube():
    b = _bench()
    for shape in ((3681, 600, 600), (3681, 900, 900), (3681, 200, 200), (50, 3, 130)):
        boxes = b.dump_boxes(shape)
        assert boxes == b.dump_boxes(shape)
        for z0, z1, y0, y1, x0, x1 in boxes:
            assert 0 <= z0 < z1 <= shape[0] and 0 <= y0 < y1 <= shape[1] and 0 <= x0 < x1 <= shape[2]
        nvox = sum((z1 - z0) * (y1 - y0) * (x1 - x0) for z0, z1, y0, y1, x0, x1 in boxes)
        # eight cubes in float32, four maps of at most 1024 x 1024 and the index in float64
        assert 8 * 4 * nvox + 8 * nvox + 4 * 4 * 1024 ** 2 <= b.DUMP_MAX_BYTES
    assert b.dump_boxes((3681, 600, 600)) != b.dump_boxes((3681, 900, 900))


def test_dump_reads_sparse_lists_at_the_sample():
    """A local-maximum cube held as a list: the sample's voxels that are in the list carry their
    values, the others zero -- what the dense cube holds there."""
    b = _bench()
    shape = (40, 12, 16)
    rng = np.random.default_rng(1)
    dense = np.where(rng.random(shape) < 0.1, rng.random(shape), 0.0).astype(np.float32)

    class Listed:
        def __init__(self, d):
            self.shape = d.shape
            self.idx = np.flatnonzero(d)
            self.val = d.reshape(-1)[self.idx]

        def entries(self):
            return self.idx, self.val

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        b.dump_outputs(tmp, {"cube_local_max": Listed(dense),
                             "cube_local_min": Listed(np.zeros(shape, np.float32))},
                       {"maxmap": dense.max(axis=0)}, {"thresO2": [1.5, 2.5]})
        index = np.load(os.path.join(tmp, "sample_index.npy"))
        got = np.load(os.path.join(tmp, "cube_local_max.npy"))
        assert index.dtype == np.float64 and got.dtype == np.float32
        assert np.array_equal(got, dense.reshape(-1)[index.astype(np.int64)])
        assert got.any() and not np.load(os.path.join(tmp, "cube_local_min.npy")).any()
        assert np.load(os.path.join(tmp, "maxmap.npy")).dtype == np.float32
        assert np.load(os.path.join(tmp, "thresO2.npy")).dtype == np.float64
