"""GPU: `mobi_lidar_overlay` / `du.overlay_lidar_batch` -- the test bench's lidar-on-camera overlays of a batch in one call --
against the float64 restatement in tests/overlay_ref.py on synthetic sweeps (nominal beam angles plus noise, uniform depth codes,
about 20 % empty) and pinhole cameras looking along +x.

The engine works in fp32, the reference in fp64, so a point whose fate a last-bit difference may decide (overlay_ref's *fragile*
points: u or v within 2e-3 px of an integer, d within 1e-3 of 1.4 or 54, |q.z| < 1e-3) is excused: the pixels inside its marker, at
either of its possible positions, are left out.  Everywhere else a pixel equals the frame where the frame shows, and where a marker
shows it is the LUT colour of the same winning point, its index within 1 of the reference's (t * 256 may sit on an integer).  The
cases are fair by the reference alone (`overlay_ref.condition`, asserted before any device result is looked at): fragile points at
most 3 % of the kept ones per picture, left-out pixels at most 25 % of the marker-covered ones.
"""
import numpy as np
import pytest
import torch

from tests import overlay_ref as R

pytestmark = pytest.mark.gpu

# frame H, W, focal length: 37 x 53 has rows of 159 bytes (no multiple of 4: the picture ends in a short group) and H * W odd
SIZES = {"37x53": (37, 53, 150.0), "90x160": (90, 160, 80.0)}
POINT_SIZES = (1, 3, 5)


def make_case(name, seed=0):
    """B = 3 objects = 6 pictures: sweeps, matrices and frames on the host.  Even pictures take an fp32 planar frame, odd ones a uint8
    frame inside a larger buffer; picture 4's camera faces away (no kept point), picture 5's sweep holds one return."""
    H, W, focal = SIZES[name]
    rng = np.random.default_rng([seed, H, W])
    sweeps = [R.sweep(rng) for _ in range(5)] + [R.one_point_sweep(rng)]
    matrices = [R.camera(H, W, focal * (1.0 + 0.05 * i), forward=i != 4, shift=(0.3 - 0.1 * i, -0.2, 0.1 * i)) for i in range(6)]
    planar = [rng.uniform(-1.1, 1.1, (3, H, W)).astype(np.float32) for _ in range(6)]
    step = (H * W * 3 + 3) // 4 * 4 + 8                                           # frames 8 bytes apart in the larger buffer
    buffer = rng.integers(0, 256, 12 + 6 * step, dtype=np.uint8)
    offsets = [12 + i * step for i in range(6)]
    frames = [planar[i] if i % 2 == 0 else buffer[offsets[i]:offsets[i] + H * W * 3].reshape(H, W, 3) for i in range(6)]
    return dict(H=H, W=W, sweeps=sweeps, matrices=matrices, planar=planar, buffer=buffer, offsets=offsets, frames=frames)


@pytest.fixture(scope="module")
def lut():
    from mobi_amd.ldm.data import utils as du
    return du.turbo_lut()


@pytest.fixture(scope="module")
def cases(lut):
    """Per frame size: the inputs, and per point size the reference of every picture -- computed once, checked for fairness here,
    before the engine runs."""
    out = {}
    for name in SIZES:
        case = make_case(name)
        case["ref"] = {}
        for size in POINT_SIZES:
            refs = [R.reference(*case["sweeps"][i], case["matrices"][i], case["frames"][i], size, lut) for i in range(6)]
            for ref in refs:
                R.condition(ref)
            assert [r["count"] for r in refs[4:]] == [0, 1] and all(r["count"] > 300 for r in refs[:4])
            case["ref"][size] = refs
        out[name] = case
    return out


def _engine(case, size, lut):
    """One `ops.lidar_overlay` call for the case's six pictures -> (device buffer, layout)."""
    from mobi_amd import ops
    sweeps = [tuple(torch.from_numpy(a).cuda() for a in s) for s in case["sweeps"]]
    buffer = torch.from_numpy(case["buffer"]).cuda()
    frames = [torch.from_numpy(case["planar"][i]).cuda() if i % 2 == 0 else (buffer, case["offsets"][i]) for i in range(6)]
    return ops.lidar_overlay(sweeps, case["matrices"], frames, torch.from_numpy(lut).cuda(), H=case["H"], W=case["W"], point_size=size)


@pytest.mark.parametrize("size", POINT_SIZES)
@pytest.mark.parametrize("name", list(SIZES))
def test_pictures_and_records_against_float64(cases, lut, name, size):
    case, refs = cases[name], cases[name]["ref"][size]
    H, W = case["H"], case["W"]
    out, layout = _engine(case, size, lut)
    again, _ = _engine(case, size, lut)
    differ = torch.nonzero(out != again).reshape(-1)
    assert differ.numel() == 0, differ[:16].tolist()                                # two calls, bit-equal buffers
    flat = out.cpu().numpy()
    rec = flat[layout["records"]:layout["bytes"]].view(np.uint32).reshape(6, 4)
    for i, ref in enumerate(refs):
        o = layout["pictures"][i][0]
        pic = flat[o:o + H * W * 3].reshape(H, W, 3)
        zmin, zmax = rec[i, :2].copy().view(np.float32)
        print(f"{name} point_size {size} picture {i}: kept {rec[i, 2]} (reference {ref['count']}, fragile {int(ref['fragile'].sum())}), "
              f"z {zmin:.6g} .. {zmax:.6g} (reference {ref['zmin']} .. {ref['zmax']}), left out {int(ref['left_out'].sum())} of "
              f"{int(ref['covered'].sum())} covered pixels")
        R.check_record(zmin, zmax, rec[i, 2], ref, f"picture {i}")
        R.check_picture(pic, ref, lut, f"picture {i}")
        assert rec[i, 3] == 0
    assert np.array_equal(flat[layout["pictures"][4][0]:][:H * W * 3].reshape(H, W, 3), refs[4]["frame"])     # no kept point: the frame
    assert rec[5, 2] == 1 and rec[5, 0] == rec[5, 1]                                # one kept point: zmax == zmin, the LUT's entry 0
    one = flat[layout["pictures"][5][0]:][:H * W * 3].reshape(H, W, 3)
    drawn = refs[5]["key"] > 0
    assert (one[drawn] == lut[0]).all() and drawn.sum() == len(R.marker_offsets(size))


def test_the_python_layer_splits_a_large_batch(cases, lut):
    """B = 33 objects = 66 pictures at 37 x 53 through `du.overlay_lidar_batch`: more than one engine call holds; every picture equals
    the same picture made alone."""
    from mobi_amd.ldm.data import utils as du
    case = cases["37x53"]
    H, W, P = case["H"], case["W"], 66
    pick = [i % 6 for i in range(P)]
    depth, pitch, yaw = (torch.from_numpy(np.stack([case["sweeps"][i][k] for i in pick])).cuda() for k in range(3))
    matrices = np.stack([R.camera(H, W, 150.0 + 0.5 * i, shift=(0.01 * i, -0.2, 0.1)) for i in range(P)])
    buffer = torch.from_numpy(case["buffer"]).cuda()
    planar = [torch.from_numpy(case["planar"][i]).cuda() if i % 2 == 0 else None for i in pick]
    offsets = [None if i % 2 == 0 else case["offsets"][i] for i in pick]
    pics, rec = du.overlay_lidar_batch(depth=depth, pitch=pitch, yaw=yaw, lidar2image=matrices, frames_f32=planar,
                                       frames_u8=(buffer, offsets), size=(H, W))
    assert len(pics) == P and rec["count"].shape == (P,) and (rec["count"][[i for i in range(P) if i % 6 != 5]] > 300).all()
    for i in range(P):
        alone, rec1 = du.overlay_lidar_batch(depth=depth[i:i + 1], pitch=pitch[i:i + 1], yaw=yaw[i:i + 1], lidar2image=matrices[i:i + 1],
                                             frames_f32=planar[i:i + 1], frames_u8=(buffer, offsets[i:i + 1]), size=(H, W))
        assert np.array_equal(alone[0], pics[i]), i
        assert all(rec1[k][0] == rec[k][i] for k in ("zmin", "zmax", "count")), i
    frame = R.frame_u8(case["frames"][0])
    assert (pics[0] != frame).any(-1).sum() > 100 and (pics[0] == frame).all(-1).sum() > 100


def test_the_recomposed_frame_is_read_in_place(lut):
    """The command's path: `du.export_camera_batch(..., return_device=True)` leaves the recomposed frames in its device buffer; the
    overlay drawn on them there equals the overlay drawn on a copy."""
    from mobi_amd.ldm.data import utils as du
    from oracle import weights as Wt
    H, W, ps, n = 90, 160, 64, 2
    g = lambda what, shape: torch.clamp(Wt.synth_input(f"lo.{what}", shape) * 0.5, -1, 1).cuda()
    mask = torch.ones(n, H, W)
    mask[0, 20:70, 40:130] = 0
    mask[1, 0:40, 0:50] = 0
    pictures, buf, layout = du.export_camera_batch(patch_pred=g("pred", (n, 3, ps, ps)), patch_gt=g("gt", (n, 3, ps, ps)),
                                                   ref_image=Wt.synth_input("lo.ref", (n, 3, 224, 224)).cuda(), image=g("image", (n, 3, H, W)),
                                                   mask=mask.cuda(), crop=[(30, 10, 101, 77), (0, 0, 67, 53)], frames=True, return_device=True)
    assert buf.is_cuda and buf.dtype == torch.uint8 and buf.numel() == layout["bytes"]
    again = du.export_camera_batch(patch_pred=g("pred", (n, 3, ps, ps)), patch_gt=g("gt", (n, 3, ps, ps)),
                                   ref_image=Wt.synth_input("lo.ref", (n, 3, 224, 224)).cuda(), image=g("image", (n, 3, H, W)),
                                   mask=mask.cuda(), crop=[(30, 10, 101, 77), (0, 0, 67, 53)], frames=True)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(pictures, again) for k in a)            # the default return is unchanged
    rng = np.random.default_rng(17)
    sweeps = [R.sweep(rng) for _ in range(n)]
    depth, pitch, yaw = (torch.from_numpy(np.stack([s[k] for s in sweeps])).cuda() for k in range(3))
    matrices = np.stack([R.camera(H, W, 80.0), R.camera(H, W, 95.0)])
    offsets = [entry["frame"][0] for entry in layout["objects"]]
    in_place, rec = du.overlay_lidar_batch(depth=depth, pitch=pitch, yaw=yaw, lidar2image=matrices, frames_u8=(buf, offsets), size=(H, W))
    copy = torch.cat([torch.zeros(16, dtype=torch.uint8)] + [torch.from_numpy(p["frame"].copy()).reshape(-1) for p in pictures]).cuda()
    copied, rec2 = du.overlay_lidar_batch(depth=depth, pitch=pitch, yaw=yaw, lidar2image=matrices,
                                          frames_u8=(copy, [16, 16 + H * W * 3]), size=(H, W))
    for i in range(n):
        assert np.array_equal(in_place[i], copied[i]) and rec["count"][i] == rec2["count"][i] > 300
        ref = R.reference(*sweeps[i], matrices[i], pictures[i]["frame"], 3, lut)
        R.check_picture(in_place[i], ref, lut, f"object {i}")
