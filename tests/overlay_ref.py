"""A helper, not a test: the lidar-on-camera overlay of ONE picture restated in float64 numpy ("lidar-on-camera overlays";
include/mobi_engine.h, mobi_lidar_overlay), the synthetic sweeps and cameras the overlay tests share, and per sweep pixel whether
the point is *fragile*: one whose fate a last-bit difference between fp32 and fp64 may decide --
    u or v within 2e-3 px of an integer (the frame's edges included), d within 1e-3 of 1.4 or 54, or |q.z| < 1e-3."""
import numpy as np

H0, W0 = 32, 1096
D_MIN, D_MAX = 1.4, 54.0
EPS_PX, EPS_D, EPS_Z = 2e-3, 1e-3, 1e-3


def marker_offsets(point_size):
    r = point_size // 2
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= (point_size / 2) ** 2]


def frame_u8(frame):
    """uint8 [H, W, 3] as it is; fp32 [3, H, W] in [-1, 1] -> (x + 1) / 2 * 255, clamped, truncated.  This one step is in fp32, not
    fp64, and is the same numpy expression as the product's `du.frame_u8`: the definition asks for the fp32 result bit for bit
    (a truncation has no tolerance to give), so for frame pixels this helper is independent of the HIP kernel, which is what the
    tests compare it with, but not of the product's numpy definition."""
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        return frame.copy()
    x = frame.astype(np.float32)
    return ((x + np.float32(1)) / np.float32(2) * np.float32(255)).clip(0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def reference(depth, pitch, yaw, matrix, frame, point_size, lut):
    """depth / pitch / yaw fp32 [H0, W0], matrix 4 x 4 (taken through fp32, as the engine is handed it), frame uint8 [H, W, 3] or fp32
    [3, H, W] -> dict:
      picture uint8 [H, W, 3]; key int [H, W] = the winning point's sweep index + 1 (0: the frame shows); lut_index int [H0 * W0]
      (-1: not kept); kept / fragile bool [H0 * W0]; left_out bool [H, W] = inside the marker of a fragile point at either of its
      possible positions; covered bool [H, W] = under any marker (or left out); zmin, zmax, count over the kept points and
      zmin_firm, zmax_firm over the kept points that are not fragile (None when there is none)."""
    pic = frame_u8(frame)
    H, W = pic.shape[:2]
    m = np.asarray(matrix, dtype=np.float64).reshape(-1, 4)[:3].astype(np.float32).astype(np.float64)
    code, pitch, yaw = (np.asarray(a, dtype=np.float32).astype(np.float64).reshape(-1) for a in (depth, pitch, yaw))
    d = (code + 1.0) / 2.0 * 54.0
    x, y, z = np.cos(yaw) * np.cos(pitch) * d, -np.sin(yaw) * np.cos(pitch) * d, np.sin(pitch) * d
    q = [m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3)]
    zc = np.clip(q[2], 1e-5, 1e5)
    u, v = q[0] / zc, q[1] / zc
    kept = (d > D_MIN) & (d < D_MAX) & (q[2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    near = lambda a: np.abs(a - np.rint(a)) < EPS_PX
    candidate = ((d > D_MIN - EPS_D) & (d < D_MAX + EPS_D) & (q[2] > -EPS_Z) & (u > -EPS_PX) & (u < W + EPS_PX) & (v > -EPS_PX)
                 & (v < H + EPS_PX))
    fragile = candidate & (near(u) | near(v) | (np.abs(d - D_MIN) < EPS_D) | (np.abs(d - D_MAX) < EPS_D) | (np.abs(q[2]) < EPS_Z))
    offsets = marker_offsets(point_size)
    index = np.nonzero(kept)[0]
    key = np.zeros((H, W), dtype=np.int64)
    lut_index = np.full(code.shape, -1, dtype=np.int64)
    out = {"kept": kept, "fragile": fragile, "count": int(kept.sum()), "zmin": None, "zmax": None, "zmin_firm": None, "zmax_firm": None,
           "near_plane": candidate & (np.abs(q[2]) < EPS_Z)}
    if len(index):
        zk = zc[index]
        zmin, zmax = zk.min(), zk.max()
        t = (zk - zmin) / (zmax - zmin) if zmax != zmin else np.zeros_like(zk)
        lut_index[index] = np.minimum((t * 256).astype(np.int64), 255)
        px, py = np.floor(u[index]).astype(np.int64), np.floor(v[index]).astype(np.int64)
        for dx, dy in offsets:
            xx, yy = px + dx, py + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            np.maximum.at(key, (yy[ok], xx[ok]), index[ok] + 1)
        out.update(zmin=zmin, zmax=zmax)
        firm = kept & ~fragile
        if firm.any():
            out.update(zmin_firm=zc[firm].min(), zmax_firm=zc[firm].max())
    drawn = key > 0
    pic[drawn] = np.asarray(lut)[lut_index[key[drawn] - 1]]
    left_out = np.zeros((H, W), dtype=bool)
    for i in np.nonzero(fragile)[0]:
        for fx in {int(np.floor(u[i] - EPS_PX)), int(np.floor(u[i] + EPS_PX))}:
            for fy in {int(np.floor(v[i] - EPS_PX)), int(np.floor(v[i] + EPS_PX))}:
                for dx, dy in offsets:
                    if 0 <= fx + dx < W and 0 <= fy + dy < H:
                        left_out[fy + dy, fx + dx] = True
    out.update(picture=pic, key=key, lut_index=lut_index, left_out=left_out, covered=drawn | left_out, frame=frame_u8(frame))
    return out


def condition(ref):
    """What makes a picture a fair case, from the reference alone: fragile points at most 3 % of the kept points, left-out pixels at
    most 25 % of the marker-covered ones, no point on the camera's plane, and a depth range that no fragile point sets."""
    n_fragile = int(ref["fragile"].sum())
    assert not ref["near_plane"].any()
    assert n_fragile <= 0.03 * ref["count"], (n_fragile, ref["count"])
    assert ref["left_out"].sum() <= 0.25 * max(int(ref["covered"].sum()), 1), (int(ref["left_out"].sum()), int(ref["covered"].sum()))
    assert ref["zmin"] == ref["zmin_firm"] and ref["zmax"] == ref["zmax_firm"]


def check_picture(pic, ref, lut, what=""):
    """pic against `reference`'s result pixel by pixel: pixels inside a fragile point's marker are left out; every other pixel equals
    the frame where the frame shows, and where a marker shows it is the LUT colour of the same winning point with an index within
    1 of the reference's."""
    lut = np.asarray(lut)
    check = ~ref["left_out"]
    shows_frame = check & (ref["key"] == 0)
    assert np.array_equal(pic[shows_frame], ref["frame"][shows_frame]), what
    marker = check & (ref["key"] > 0)
    idx = ref["lut_index"][ref["key"][marker] - 1]
    ok = np.zeros(idx.shape, dtype=bool)
    for step in (-1, 0, 1):
        ok |= (pic[marker] == lut[np.clip(idx + step, 0, 255)]).all(-1)
    assert ok.all(), (what, int((~ok).sum()), int(marker.sum()))
    return int(marker.sum())


def check_record(zmin, zmax, count, ref, what=""):
    """The kept count within the fragile points; zmin and zmax within 1e-5 relative of the reference's value, or of its value
    without its fragile points."""
    assert abs(int(count) - ref["count"]) <= int(ref["fragile"].sum()), what
    if ref["count"] == 0 and count == 0:
        assert zmin == 0 and zmax == 0, what
        return
    for got, names in ((zmin, ("zmin", "zmin_firm")), (zmax, ("zmax", "zmax_firm"))):
        wants = [ref[n] for n in names if ref[n] is not None]
        assert any(abs(float(got) - w) <= 1e-5 * abs(w) for w in wants), (what, names[0], float(got), wants)


def camera(H, W, focal, forward=True, shift=(0.3, -0.2, 0.1)):
    """4 x 4 lidar2image of a pinhole camera looking along +x of the lidar frame, principal point at the frame's centre, `shift`
    metres from the lidar.  forward=False: it faces away from the sweep -- straight up, where no beam points (a sweep goes all
    the way round, so a camera looking along -x would still see half of it)."""
    rot = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])         # camera x = right, y = down, z = ahead
    if not forward:
        rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ext = np.eye(4)
    ext[:3, :3], ext[:3, 3] = rot, rot @ -np.asarray(shift)
    k = np.eye(4)
    k[0, 0] = k[1, 1] = focal
    k[0, 2], k[1, 2] = W / 2.0, H / 2.0
    return k @ ext


def sweep(rng, empty=0.2):
    """fp32 depth code, pitch, yaw [H0, W0]: nominal beam angles (pitch +10 .. -30 degrees down the rows, yaw pi .. -pi along the
    columns) plus small noise, depth codes uniform, about `empty` of them -1 (no return)."""
    pitch = np.deg2rad(np.linspace(10.0, -30.0, H0))[:, None] + rng.normal(0, 2e-3, (H0, W0))
    yaw = np.linspace(np.pi, -np.pi, W0, endpoint=False)[None, :] + rng.normal(0, 1e-3, (H0, W0))
    code = rng.uniform(-0.95, 1.0, (H0, W0))
    code[rng.uniform(size=(H0, W0)) < empty] = -1.0
    return code.astype(np.float32), pitch.astype(np.float32), yaw.astype(np.float32)


def one_point_sweep(rng, row=8, column=W0 // 2 + 3, code=0.1):
    """A sweep whose only return is one pixel near yaw 0 (ahead of a forward camera)."""
    _, pitch, yaw = sweep(rng)
    depth = np.full((H0, W0), -1.0, dtype=np.float32)
    depth[row, column] = code
    return depth, pitch, yaw
