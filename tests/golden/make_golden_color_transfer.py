#!/usr/bin/env python3
"""Generate tests/golden/g26_color_transfer_ot.npz from the REFERENCE's own CTSOT (TextureTools/texturetools/image/color_transfer_ot.py):

    python tests/golden/make_golden_color_transfer.py <reference root> [output directory]

The reference's module is loaded from its file with `cv2` stubbed as an empty module (it is only touched by the regulariser, and every call here passes
reg_sigmaXY=0.0, so no OpenCV code runs).  Two cases, random float32 images from a seeded numpy generator:
    a: 37 x 29 x 3, steps 3, batch 2        b: 16 x 9 x 4, steps 2, batch 5
Stored per case: src, dst, the directions the reference drew (recorded by drawing them again from the same seed, in the reference's order and arithmetic, and
checked against what a patched np.random.normal saw), steps, batch, and the reference's output.  Asserted: no two projections of any batch are equal, for the
source and for the target -- the fixture must not depend on the order numpy's argsort gives to ties."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.support import color_transfer_ref as R  # noqa: E402

CASES = (("a", 37, 29, 3, 3, 2, 2601), ("b", 16, 9, 4, 2, 5, 2602))


def load_reference(root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    path = os.path.join(root, "TextureTools", "texturetools", "image", "color_transfer_ot.py")
    spec = importlib.util.spec_from_file_location("reference_color_transfer_ot", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root, outdir):
    ref = load_reference(root)
    out = {}
    for name, H, W, C, steps, batch, seed in CASES:
        rng = np.random.default_rng(seed)
        src = rng.uniform(0.0, 1.0, (H, W, C)).astype(np.float32)
        dst = (rng.uniform(0.0, 1.0, (H, W, C)) ** 2 * 0.8 + 0.1).astype(np.float32)
        # the directions the reference is about to draw: the same calls on the same seed
        np.random.seed(seed)
        dirs = np.empty((steps * batch, C), np.float32)
        for k in range(steps * batch):
            d = np.random.normal(size=(C,)).astype(np.float32)
            dirs[k] = d / np.linalg.norm(d, axis=-1)
        # ... and what it does draw, seen through np.random.normal
        seen, normal = [], np.random.normal

        def spy(*a, **k):
            v = normal(*a, **k)
            seen.append(v.astype(np.float32))
            return v
        np.random.seed(seed)
        np.random.normal = spy
        try:
            res = ref.CTSOT(src.copy(), dst.copy(), steps=steps, batch_size=batch, reg_sigmaXY=0.0)
        finally:
            np.random.normal = normal
        assert res.dtype == np.float32 and res.shape == (H, W, C) and len(seen) == steps * batch
        for k, v in enumerate(seen):
            assert (v / np.linalg.norm(v, axis=-1)).tobytes() == dirs[k].tobytes()
        ties = []
        mine = R.ot_loop(src, dst, dirs, steps, batch, ties=ties)
        assert all(t == (0, 0) for t in ties), "%s: equal projections %s: the fixture would depend on argsort's tie order" % (name, ties)
        assert mine.tobytes() == res.tobytes(), "%s: the sequential float32 restatement differs from the reference in %d values" % (name, int((mine != res).sum()))
        out.update({name + "_src": src, name + "_dst": dst, name + "_dirs": dirs, name + "_steps": np.int32(steps), name + "_batch": np.int32(batch),
                    name + "_out": res})
        print("%s: %d x %d x %d, steps %d, batch %d: no ties, restatement bit-equal, max |out - src| = %.3g" % (name, H, W, C, steps, batch, np.abs(res - src).max()))
    path = os.path.join(outdir, "g26_color_transfer_ot.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
