"""utx_rasterize / utx_interpolate against the independent restatement of the rule (tests/support/raster_exact_ref.py), bit for bit.

The restatement shares no code with oracle/geom_ref.c (numpy float32 + Python integers) and is itself checked against exact
arithmetic in tests/test_raster_exact_cpu.py.  Coverage and ids are integers and the float steps have one order: nothing is
tolerated, every one of the H x W x 4 values has to have the restatement's bits.  The case sets put pixel centres on shared edges and
vertices, coordinates on half sub-pixel units, many triangles at one depth, the 2048-pixel switch to the queued kernel and more
queued triangles than that kernel has workgroups, 1 x N images, a clear pass longer than its grid, perspective weights, and
vertices outside the accepted range or not finite."""
import numpy as np
import pytest
import torch

from tests.support import raster_exact_ref as R

pytestmark = pytest.mark.gpu


def _gpu_raster(case):
    from unitex_amd.texturetools import ops
    r = ops.rasterize(torch.from_numpy(case.pos).cuda(), torch.from_numpy(case.tri).cuda(), case.H, case.W)
    torch.cuda.synchronize()
    return r


def _same_bits(got, ref, what):
    a, b = R.bits(got), R.bits(ref)
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, "%s: %d of %d values differ, first at %s: 0x%08x vs 0x%08x" % (
        what, bad.shape[0], a.size, tuple(int(v) for v in bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.all_cases()])
def test_rasterize_equals_the_rule(case):
    ref, _ = R.rule_of(case)
    got = _gpu_raster(case).cpu().numpy()
    nan_records = int(np.isnan(got[..., 2]).sum())
    assert nan_records == 0, "%s: %d records carry a NaN z/w" % (case.name, nan_records)
    _same_bits(got, ref, case.name)


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.all_cases() if c.attrs])
def test_interpolate_equals_the_rule(case, C):
    from unitex_amd.texturetools import ops
    rast, _ = R.rule_of(case)
    attr = R.attrs_of(case, C)
    ref = R.interpolate_rule(attr, rast, case.tri)
    got = ops.interpolate(torch.from_numpy(attr).cuda(), torch.from_numpy(np.array(rast)).cuda(), torch.from_numpy(case.tri).cuda()).cpu().numpy()
    _same_bits(got, ref, "%s C=%d" % (case.name, C))
    assert not got[rast[..., 3] == 0].any(), "zeros where the pixel is empty"


def test_queue_switch_does_not_move_pixels():
    """the 4 x 513 triangle with its first row above the image (clipped box 2048 pixels: one thread scans it) and one pixel lower
    (2052 pixels: queued, a workgroup scans it) gives the same records, one row apart"""
    by = {c.name: c for c in R.case_set("queue")}
    up = _gpu_raster(by["queue-shift-up"]).cpu().numpy()
    down = _gpu_raster(by["queue-shift-down"]).cpu().numpy()
    assert (down[1:513, :, 3] > 0).sum() > 1000
    _same_bits(down[1:513], up[:512], "shifted across BIG_BBOX")


def test_image_size_beyond_the_range_is_refused():
    """H, W <= 2^22 is part of the accepted range (pixel centres stay within 2^30 sub-pixel units): a larger size is an error, before any launch"""
    from unitex_amd.texturetools import ops
    from unitex_amd._lib import ptr
    ctx = ops.get_ctx(0)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    tri = torch.zeros(3, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="utx_rasterize"):
        ctx.check(ctx.lib.utx_rasterize(ctx.handle, ptr(buf), ptr(tri), 1, (1 << 22) + 1, 1, ptr(buf), ptr(buf), ctx.stream()))
