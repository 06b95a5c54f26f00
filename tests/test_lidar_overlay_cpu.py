"""CPU: the lidar-on-camera overlays' host side -- `mobi_lidar_overlay`'s struct and refusals (host checks: no launch),
`ops.lidar_overlay_layout`, and the numpy definition on hand-made cases."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_struct_ids_and_sizes(lib):
    from mobi_amd import _lib
    assert lib.mobi_struct_size(33) == C.sizeof(_lib.LidarOverlayParams) == 80 and _lib.STRUCT_IDS[33] is _lib.LidarOverlayParams
    assert lib.mobi_struct_size(34) == C.sizeof(_lib.LidarOverlayPicture) == 104 and _lib.STRUCT_IDS[34] is _lib.LidarOverlayPicture
    assert lib.mobi_abi_version() == 6
    assert "mobi_lidar_overlay" in _lib.SYMBOLS and "mobi_lidar_overlay_workspace_bytes" in _lib.SYMBOLS
    # a u32 key per frame pixel (rows of keys padded to whole groups of four) and a 16-byte record, per picture
    assert lib.mobi_lidar_overlay_workspace_bytes(6, 37, 53) == 6 * (1964 * 4 + 16)
    assert lib.mobi_lidar_overlay_workspace_bytes(16, 900, 1600) == 16 * (900 * 1600 * 4 + 16)
    assert lib.mobi_lidar_overlay_workspace_bytes(0, 37, 53) == 0 and lib.mobi_lidar_overlay_workspace_bytes(2, 0, 53) == 0


def test_lidar_overlay_validates_before_any_launch(lib):
    """No GPU here: every call must return on the host."""
    from mobi_amd import _lib, ops
    H, W, P = 37, 53, 3
    lay = ops.lidar_overlay_layout(P, H, W)
    need = lib.mobi_lidar_overlay_workspace_bytes(P, H, W)

    def call(n=P, out_bytes=lay["bytes"], records=lay["records"], shift=0, ws_bytes=need, point_size=3, kind=1, frame_offset=8,
             null=None, null_picture=None, H=H, W=W, h0=32, w0=1096, out=4096, ws=4096, sweep=4096, frame=1 << 20, same=None):
        pics = (_lib.LidarOverlayPicture * max(n, 1))()
        for i, pic in enumerate(pics):
            pic.depth = pic.pitch = pic.yaw = sweep
            pic.frame, pic.frame_offset, pic.frame_kind = frame, frame_offset, kind
            pic.out_offset = lay["pictures"][min(i, P - 1)][0] + shift
            pic.matrix[:] = [1.0] * 12
        if null_picture:
            setattr(pics[n - 1], null_picture, None)
        if same:                                                                    # picture same[0] where picture same[1] is, plus a shift
            pics[same[0]].out_offset = pics[same[1]].out_offset + same[2]
        p = _lib.LidarOverlayParams()
        p.pictures, p.lut, p.out, p.workspace = C.addressof(pics), 4096, out, ws
        p.out_bytes, p.records_offset, p.workspace_bytes = out_bytes, records, ws_bytes
        p.n_pictures, p.h0, p.w0, p.H, p.W, p.point_size = n, h0, w0, H, W, point_size
        if null:
            setattr(p, null, None)
        return lib.mobi_lidar_overlay(C.byref(p), None)

    assert lib.mobi_lidar_overlay(None, None) == -1
    for name in ("pictures", "lut", "out", "workspace"):
        assert call(null=name) == -1, name                                          # null pointers
    for name in ("depth", "pitch", "yaw", "frame"):
        assert call(null_picture=name) == -1, name
    assert call(n=0) == -1 and call(n=65, ws_bytes=1 << 40, out_bytes=1 << 40) == -2                # P of 0, or more than 64
    assert call(H=0) == -1 and call(W=-3) == -1 and call(h0=0) == -1 and call(w0=0) == -1
    assert call(out_bytes=lay["bytes"] - 4) == -1                                   # the records run past out_bytes
    assert call(out_bytes=lay["records"] - 4, records=0) == -1                      # a picture does
    assert call(shift=-4) == -1 and call(records=-16) == -1                         # negative offsets
    assert call(frame_offset=-4) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1                 # a workspace that is too small
    assert call(shift=2, out_bytes=lay["bytes"] + 4) == -4                          # misaligned offsets and pointers
    assert call(records=lay["records"] + 2, out_bytes=lay["bytes"] + 4) == -4
    assert call(frame_offset=6) == -4 and call(out=4098) == -4 and call(ws=4104) == -4 and call(sweep=4098) == -4
    for bad in (0, 2, 4, 7, -1):
        assert call(point_size=bad) == -2, bad                                      # point_size outside {1, 3, 5}
    assert call(kind=2) == -1 and call(kind=-1) == -1                               # an unknown frame kind
    # overlaps (checked before the pointers' alignment: `ok` is a call whose only fault is a misaligned sweep pointer, so that a
    # layout the checks accept still returns on the host)
    ok = lambda **kw: call(sweep=4098, **kw) == -4
    assert ok() and call(same=(2, 0, 0)) == -1 and call(same=(1, 2, 4)) == -1       # two pictures that share bytes
    # the byte behind a 37 x 53 picture (5883 bytes) is the picture's too: the records may not start inside it, only behind it
    assert call(records=lay["pictures"][2][0] + 5880) == -1 and ok(records=lay["pictures"][2][0] + 5884)
    base = 1 << 16                                                                  # a frame source inside `out`, and next to it
    assert call(out=base, frame=base + 400, frame_offset=0) == -1 and call(out=base, frame=base - 5880, frame_offset=0) == -1
    assert ok(out=base, frame=base - 5884, frame_offset=0) and ok(out=base, frame=base + lay["bytes"], frame_offset=0)
    assert call(out=base, frame=base - 12 * H * W + 4, frame_offset=0, kind=0) == -1 and ok(out=base, frame=base - 12 * H * W, frame_offset=0, kind=0)


def test_lidar_overlay_layout():
    from mobi_amd import ops
    for P, H, W in ((6, 37, 53), (1, 1, 1), (64, 90, 160), (66, 37, 53)):
        lay = ops.lidar_overlay_layout(P, H, W)
        assert len(lay["pictures"]) == P and all(shape == (H, W, 3) for _, shape in lay["pictures"])
        spans = [(o, o + H * W * 3) for o, _ in lay["pictures"]] + [(lay["records"], lay["records"] + 16 * P)]
        assert all(lo % 4 == 0 for lo, _ in spans) and max(hi for _, hi in spans) == lay["bytes"]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                  # in order, no overlaps, the records last
    for bad in ((0, 37, 53), (2, 0, 53), (2, 37, -1)):
        with pytest.raises(ValueError):
            ops.lidar_overlay_layout(*bad)


# a camera at the lidar's origin looking along +x: u = 10 * (-y / x) + 8, v = 10 * (-z / x) + 6 on a 12 x 16 frame
CAMERA = np.array([[8.0, -10.0, 0.0, 0.0], [6.0, 0.0, -10.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
LUT = np.stack([np.arange(256), 255 - np.arange(256), np.full(256, 7)], axis=1).astype(np.uint8)


def _at(u, v, depth):
    """The lidar point that CAMERA projects to (u, v) at camera depth `depth`."""
    return [depth, -(u - 8.0) / 10.0 * depth, -(v - 6.0) / 10.0 * depth]


def test_numpy_definition_on_hand_made_cases():
    from mobi_amd.ldm.data import utils as du
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
    planar = rng.uniform(-1.2, 1.2, (3, 12, 16)).astype(np.float32)
    assert [len(du.marker_offsets(s)) for s in (1, 3, 5)] == [1, 9, 21]
    for bad in (0, 2, 4):
        with pytest.raises(ValueError):
            du.marker_offsets(bad)
    # one point, each point size: the marker's pixels take the LUT's entry 0 (zmax == zmin), every other pixel is the frame
    for size, shape in ((1, ["#"]), (3, ["###"] * 3), (5, [".###.", "#####", "#####", "#####", ".###."])):
        pic, rec = du.overlay_lidar_on_image([_at(7.5, 5.5, 4.0)], CAMERA, frame, point_size=size, lut=LUT, return_record=True)
        drawn = np.zeros((12, 16), dtype=bool)
        r = size // 2
        for dy, row in enumerate(shape):
            for dx, c in enumerate(row):
                drawn[5 - r + dy, 7 - r + dx] = c == "#"
        assert drawn.sum() == {1: 1, 3: 9, 5: 21}[size]
        assert (pic[drawn] == LUT[0]).all() and np.array_equal(pic[~drawn], frame[~drawn]), size
        assert rec == (np.float32(4.0), np.float32(4.0), 1)
    # a marker clipped at a corner: (0.5, 0.5) with point_size 5 keeps the quarter of its disc that lies inside the frame
    pic = du.overlay_lidar_on_image([_at(0.5, 0.5, 4.0)], CAMERA, frame, point_size=5, lut=LUT)
    drawn = np.zeros((12, 16), dtype=bool)
    drawn[:3, :3] = True
    drawn[2, 2] = False                                                             # dx = dy = 2: outside the radius
    assert (pic[drawn] == LUT[0]).all() and np.array_equal(pic[~drawn], frame[~drawn])
    pic = du.overlay_lidar_on_image([_at(15.5, 11.5, 4.0)], CAMERA, frame, point_size=3, lut=LUT)
    drawn = np.zeros((12, 16), dtype=bool)
    drawn[10:, 14:] = True
    assert (pic[drawn] == LUT[0]).all() and np.array_equal(pic[~drawn], frame[~drawn])
    # two overlapping points: the later one on top, in either order; colours from the depth range (t = 0 and t = 1 -> 0 and 255)
    near, far = _at(7.5, 5.5, 4.0), _at(8.5, 5.5, 8.0)
    pic, rec = du.overlay_lidar_on_image([near, far], CAMERA, frame, point_size=3, lut=LUT, return_record=True)
    assert rec == (np.float32(4.0), np.float32(8.0), 2)
    assert (pic[4:7, 7:10] == LUT[255]).all() and (pic[4:7, 6] == LUT[0]).all()
    pic = du.overlay_lidar_on_image([far, near], CAMERA, frame, point_size=3, lut=LUT)
    assert (pic[4:7, 6:9] == LUT[0]).all() and (pic[4:7, 9] == LUT[255]).all()
    # a third point half way takes entry int(0.5 * 256) = 128
    pic = du.overlay_lidar_on_image([near, far, _at(2.5, 9.5, 6.0)], CAMERA, frame, point_size=1, lut=LUT)
    assert (pic[9, 2] == LUT[128]).all()
    # zmax == zmin with several points: entry 0 everywhere
    pic = du.overlay_lidar_on_image([_at(3.5, 3.5, 5.0), _at(12.5, 8.5, 5.0)], CAMERA, frame, point_size=1, lut=LUT)
    assert (pic[3, 3] == LUT[0]).all() and (pic[8, 12] == LUT[0]).all() and (pic != frame).any(-1).sum() <= 2
    # no point at all: behind the camera, outside the frame, an empty list -- the picture is the frame
    for pts in ([], [[-4.0, 0.0, 0.0]], [_at(16.0, 5.0, 4.0)], [_at(-0.01, 5.0, 4.0)], [_at(5.0, 12.0, 4.0)]):
        pic, rec = du.overlay_lidar_on_image(np.zeros((0, 3)) if not pts else pts, CAMERA, frame, lut=LUT, return_record=True)
        assert np.array_equal(pic, frame) and rec[2] == 0
    # an fp32 planar frame: (x + 1) / 2 * 255 in fp32, clamped, truncated
    pic = du.overlay_lidar_on_image(np.zeros((0, 3)), CAMERA, planar, lut=LUT)
    want = ((planar + np.float32(1)) / np.float32(2) * np.float32(255)).clip(0, 255).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(pic, want) and pic.min() == 0 and pic.max() == 255
    # the map itself: matplotlib's turbo, 256 entries
    lut = du.turbo_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and len({tuple(c) for c in lut}) > 200


def test_numpy_definition_agrees_with_the_float64_restatement():
    """The product's fp32 definition against tests/overlay_ref.py on a synthetic sweep, outside the fragile points' markers."""
    from mobi_amd.ldm.data import utils as du
    from mobi_amd.ldm.data.lidar_converter import LidarConverter
    from tests import overlay_ref as R
    rng = np.random.default_rng(11)
    H, W = 37, 53
    depth, pitch, yaw = R.sweep(rng)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    cam = R.camera(H, W, 60.0)
    lut = du.turbo_lut()
    points = LidarConverter().range2pcd(depth, pitch, yaw)[0]
    for size in (1, 3, 5):
        ref = R.reference(depth, pitch, yaw, cam, frame, size, lut)
        pic, rec = du.overlay_lidar_on_image(points, cam, frame, point_size=size, lut=lut, return_record=True)
        R.condition(ref)
        assert ref["count"] > 500
        R.check_record(*rec, ref, f"point_size {size}")
        assert R.check_picture(pic, ref, lut, f"point_size {size}") > 100


def test_overlay_lidar_batch_refuses_frames_it_cannot_place():
    """Host checks of `du.overlay_lidar_batch` that come before any engine call."""
    import torch
    from mobi_amd.ldm.data import utils as du
    sweep = torch.zeros(2, 32, 1096)
    common = dict(depth=sweep, pitch=sweep, yaw=sweep, lidar2image=np.stack([np.eye(4)] * 2))
    with pytest.raises(ValueError, match="not \\(90, 160\\)"):                      # size against an fp32 frame's own shape
        du.overlay_lidar_batch(frames_f32=torch.zeros(2, 3, 37, 53), size=(90, 160), **common)
    with pytest.raises(ValueError, match="not \\(37, 53\\)"):                       # two fp32 frames of different shapes
        du.overlay_lidar_batch(frames_f32=[torch.zeros(3, 37, 53), torch.zeros(3, 37, 54)], **common)
    with pytest.raises(ValueError, match="no frame"):
        du.overlay_lidar_batch(frames_f32=[torch.zeros(3, 37, 53), None], **common)
    with pytest.raises(ValueError, match="size="):                                  # uint8 frames only: the size must be given
        du.overlay_lidar_batch(frames_u8=(torch.zeros(64, dtype=torch.uint8), [0, 0]), **common)
