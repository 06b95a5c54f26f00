"""fp64 interpreter of a row-chain program (TEST INFRASTRUCTURE): the contract of `mobi_row_chain_params` as the header
comment of include/mobi_engine.h states it, restated in torch float64 -- not a reading of csrc/chain.hip.

  * `decode_chain_weight(image, dtype)`: the 200-KiB chunk image of one product back to its [320][320] matrix in T, by the
    documented layout ([chunk][fragment f = 10 kk + m][lane][8], row 32 m + tau(l & 31), column 16 (2 c + kk) + 8 (l >> 5) + j).
  * a program is DESCRIBED as a list of (code, kwargs) holding the tensors themselves:
        ("load_s" | "load_r", dict(t, img_div))          ("affine", dict(scale, shift))        ("rowstats", dict(eps))
        ("product", dict(image, bias, bias_img_stride, bias_img_div, svec, fold, resid, to_s, dst, dst_img_div))
        ("adapter", dict(dst, dst_img_div))                ("store", dict(dst, dst_img_div))
    `recording_program()` returns a subclass of ops.ChainProgram that writes this description (`.desc`) while the real
    program is built by the same calls; what is launched is the base class's and unchanged.
  * `run_program` / `run_launch` interpret descriptions: products accumulate in fp64; the row state `s` is rounded to T where
    the contract says it is T (after AFFINE_S, after a TO_S product, after ADAPTER); a stored value is rounded ONCE (the
    returned reference is the unrounded fp64 value of a product, the T-valued state for ADAPTER and STORE_S); FOLD is
    rs v + cs svec + bias with (rs, cs) = (rstd, -rstd mean) of the state ROWSTATS saw; RESID consumes `r`; image indices
    are img / div for loads, stores and biases; with two programs even images run the first, odd images the second.

Nothing here calls a `mobi_*` entry point.
"""
import functools

import torch

C = 320
CHUNKS, KK, MT, LANES, VEC = 10, 2, 10, 64, 8
FLAG_NAMES = ((1, "fold"), (2, "resid"), (4, "to_s"), (8, "store"))


def decode_chain_weight(image, dtype):
    """uint8 [204,800] chunk image -> T [320, 320] (out, in).  Every element of the matrix is written exactly once."""
    img = image.reshape(-1).view(dtype).reshape(CHUNKS, KK, MT, LANES, VEC)       # fragment f = 10 kk + m: [kk][m]
    dev = image.device
    ar = lambda k: torch.arange(k, device=dev)
    lane = ar(LANES)
    i = lane % 32
    b2, b3 = (i // 4) % 2, (i // 8) % 2
    tau = i - 4 * b2 - 8 * b3 + 8 * b2 + 4 * b3                                # bits 2 and 3 swapped
    row = 32 * ar(MT)[None, None, :, None, None] + tau[None, None, None, :, None]
    col = (16 * (2 * ar(CHUNKS)[:, None, None, None, None] + ar(KK)[None, :, None, None, None])
           + 8 * (lane // 32)[None, None, None, :, None] + ar(VEC)[None, None, None, None, :])
    flat = (row * C + col).expand_as(img).reshape(-1)
    hits = torch.zeros(C * C, dtype=torch.int64, device=dev)
    hits.index_add_(0, flat, torch.ones_like(flat))
    assert bool((hits == 1).all()), "the documented layout does not cover the matrix once"
    w = torch.empty(C * C, dtype=dtype, device=dev)
    w[flat] = img.reshape(-1)
    return w.reshape(C, C)


def flag_name(flags):
    return "|".join(n for b, n in FLAG_NAMES if flags & b) or "none"


def product_flags(kw):
    return (1 if kw["fold"] else 0) | (2 if kw["resid"] else 0) | (4 if kw["to_s"] else 0) | (8 if kw["dst"] is not None else 0)


class ProgramDescription:
    """The builder methods of ops.ChainProgram, writing the plain description only (no engine object: usable without a device)."""

    def __init__(self):
        self.desc = []

    def load(self, t, which="s", img_div=1):
        self.desc.append(("load_s" if which == "s" else "load_r", dict(t=t, img_div=img_div)))
        return self

    def affine(self, scale, shift):
        self.desc.append(("affine", dict(scale=scale, shift=shift)))
        return self

    def rowstats(self, eps):
        self.desc.append(("rowstats", dict(eps=eps)))
        return self

    def product(self, cw, *, fold=False, resid=False, to_s=False, dst=None, dst_img_div=1, bias=None, bias_img_stride=0,
                bias_img_div=1):
        self.desc.append(("product", dict(image=cw.image, bias=cw.bias if bias is None else bias, bias_img_stride=bias_img_stride,
                                          bias_img_div=bias_img_div, svec=cw.svec if fold else None, fold=fold, resid=resid,
                                          to_s=to_s, dst=dst, dst_img_div=dst_img_div)))
        return self

    def adapter(self, dst, dst_img_div=1):
        self.desc.append(("adapter", dict(dst=dst, dst_img_div=dst_img_div)))
        return self

    def store(self, dst, dst_img_div=1):
        self.desc.append(("store", dict(dst=dst, dst_img_div=dst_img_div)))
        return self


@functools.lru_cache(maxsize=None)
def recording_program():
    """ops.ChainProgram that also keeps the plain description of what it was asked to build (`.desc`); what it builds and
    what is launched are the base class's."""
    from mobi_amd import ops
    D = ProgramDescription

    class RecordingChainProgram(ops.ChainProgram):
        def __init__(self):
            super().__init__()
            self.desc = []

        def load(self, t, which="s", img_div=1):
            D.load(self, t, which, img_div)
            return super().load(t, which, img_div)

        def affine(self, scale, shift):
            D.affine(self, scale, shift)
            return super().affine(scale, shift)

        def rowstats(self, eps):
            D.rowstats(self, eps)
            return super().rowstats(eps)

        def product(self, cw, **kw):
            D.product(self, cw, **kw)
            return super().product(cw, **kw)

        def adapter(self, dst, dst_img_div=1):
            D.adapter(self, dst, dst_img_div)
            return super().adapter(dst, dst_img_div)

        def store(self, dst, dst_img_div=1):
            D.store(self, dst, dst_img_div)
            return super().store(dst, dst_img_div)

    return RecordingChainProgram


def _flat(storage, dtype, device):
    return torch.empty(0, dtype=dtype, device=device).set_(storage)


def snapshot(descs):
    """-> (descriptions whose tensors, the destinations aside, are views of clones made now; memo: storage address -> clone
    of the whole storage, destinations' included).  One clone per storage, views re-made on it: a load that aliases a
    destination (the in-place post_cam form) reads what the launch read."""
    memo = {}

    def clone_of(t):
        st = t.untyped_storage()
        if st.data_ptr() not in memo:
            memo[st.data_ptr()] = _flat(st, torch.uint8, t.device).clone().untyped_storage()
        return memo[st.data_ptr()]

    def snap(k, t):
        if not torch.is_tensor(t):
            return t
        c = clone_of(t)
        return t if k == "dst" else torch.empty(0, dtype=t.dtype, device=t.device).set_(c, t.storage_offset(), t.shape, t.stride())

    return [[(code, {k: snap(k, v) for k, v in kw.items()}) for code, kw in desc] for desc in descs], memo


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def changed_inputs(descs, snaps):
    """Names of the operands a launch read that differ from their snapshots, bit for bit (an operand in a destination's
    storage is judged by `touched_outside`: its rows inside the destination change by design)."""
    dsts = {kw["dst"].untyped_storage().data_ptr() for desc in descs for _, kw in desc if torch.is_tensor(kw.get("dst"))}
    bad = []
    for k, (desc, sdesc) in enumerate(zip(descs, snaps)):
        for i, ((code, kw), (_, skw)) in enumerate(zip(desc, sdesc)):
            for name, t in kw.items():
                if name == "dst" or not torch.is_tensor(t) or t.untyped_storage().data_ptr() in dsts:
                    continue
                if not torch.equal(bits(t), bits(skw[name])):
                    bad.append(f"program {k} operation {i} ({code}) {name}")
    return bad


def touched_outside(results, memo):
    """Destination storages with an element changed outside the rows x 320 channels the results cover -> list of strings."""
    groups = {}
    for rec in results:
        groups.setdefault(rec["dst"].untyped_storage().data_ptr(), []).append(rec)
    bad = []
    for key, recs in groups.items():
        dst = recs[0]["dst"]
        live = _flat(dst.untyped_storage(), dst.dtype, dst.device)
        before = _flat(memo[key], dst.dtype, dst.device)
        mask = torch.ones(live.numel(), dtype=torch.bool, device=dst.device)
        for rec in recs:
            d = rec["dst"]
            idx = torch.arange(live.numel(), device=d.device).as_strided(d.shape, d.stride(), d.storage_offset())[..., :C]
            mask[idx[rec["img"].to(d.device) // rec["div"], rec["row"].to(d.device)].reshape(-1)] = False
        diff = (bits(live) != bits(before)) & mask
        if bool(diff.any()):
            first = int(diff.nonzero()[0])
            bad.append(f"{int(diff.sum())} elements outside the destination rows changed (first: element {first} of the storage)")
    return bad


def _d(div):
    return div if div > 1 else 1


def rows_of(t, img, row, div, dev):
    """Rows (img / div, row) of a [N, T, >= C] view -> [R, C] on dev."""
    return t.to(dev)[..., :C][img // _d(div), row]


def round_to(v, dtype):
    return v.to(dtype).double()


def adapter_rows(x, tab, img, eps):
    """x + b + sum_h sigmoid(rstd (x . a_h - mean sum a_h) + c_h) u_h with the row's LayerNorm statistics (the formula of
    test_chain_adapter), the fp32 tables of the row's image in fp64.  x [R, C]; tab: a, u [N, H, C]; c [N, H]; b [N, C]."""
    a, c, u, b = (tab[k].to(x.device).double() for k in ("a", "c", "u", "b"))
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).square().mean(-1, keepdim=True) + eps).rsqrt()
    y = torch.empty_like(x)
    for i in torch.unique(img).tolist():
        m = img == i
        z = rstd[m] * (x[m] @ a[i].T - mean[m] * a[i].sum(-1)) + c[i]
        y[m] = x[m] + b[i] + torch.sigmoid(z) @ u[i]
    return y


def run_program(desc, images, rows, dtype, adapter_tables=None, kind=None, sel=None, dev=None):
    """Interpret one program on the images of `kind` (None: all; 0 / 1: the even / odd ones) -> one dict per storing operation:
    index, code, flags, dst (the live view), div, img / row ([R] image and row index of every computed row, image-major) and
    ref ([R, C] fp64).  sel = (img, row): only those rows (of the right kind).  adapter_tables: dict a, c, u, b, eps."""
    dev = torch.device("cpu") if dev is None else dev
    if sel is None:
        imgs = torch.arange(images) if kind is None else torch.arange(kind, images, 2)
        img, row = imgs.repeat_interleave(rows), torch.arange(rows).repeat(imgs.numel())
    else:
        img, row = sel
        if kind is not None:
            keep = img % 2 == kind
            img, row = img[keep], row[keep]
    img, row = img.to(dev), row.to(dev)
    z = torch.zeros((img.numel(), C), dtype=torch.float64, device=dev)
    s, r = z, z
    rs, cs = torch.ones_like(z[:, :1]), torch.zeros_like(z[:, :1])
    ch = torch.arange(C, device=dev)
    out = []

    def stored(i, code, flags, kw, ref):
        out.append(dict(index=i, code=code, flags=flags, dst=kw["dst"], div=_d(kw["dst_img_div"]), img=img, row=row, ref=ref))

    for i, (code, kw) in enumerate(desc):
        if code == "load_s":
            s = rows_of(kw["t"], img, row, kw["img_div"], dev).double()
        elif code == "load_r":
            r = rows_of(kw["t"], img, row, kw["img_div"], dev).double()
        elif code == "affine":
            s = round_to(s * kw["scale"].to(dev).double()[img] + kw["shift"].to(dev).double()[img], dtype)
        elif code == "rowstats":
            mean = s.mean(-1, keepdim=True)
            rs = ((s - mean).square().mean(-1, keepdim=True) + kw["eps"]).rsqrt()
            cs = -rs * mean
        elif code == "product":
            w = decode_chain_weight(kw["image"].to(dev), dtype).double()
            v = s @ w.T
            if kw["fold"]:
                v = rs * v + cs * kw["svec"].to(dev).double()
            bidx = (img // _d(kw["bias_img_div"]))[:, None] * kw["bias_img_stride"] + ch[None, :]
            v = v + kw["bias"].to(dev).double().reshape(-1)[bidx]
            if kw["resid"]:
                v, r = v + r, z
            if kw["to_s"]:
                s = round_to(v, dtype)
            if kw["dst"] is not None:
                stored(i, code, product_flags(kw), kw, v)
        elif code == "adapter":
            s = round_to(adapter_rows(s, adapter_tables, img, adapter_tables["eps"]), dtype)
            stored(i, code, 8, kw, s)
        elif code == "store":
            stored(i, code, 0, kw, s)
        else:
            raise ValueError(f"chain_ref: no operation {code!r}")
    return out


def run_launch(descs, images, rows, dtype, adapter_tables=None, sel=None, dev=None):
    """One launch: one program on every image, or two on the even / odd images -> the results of every storing operation, each
    with `prog` (0 / 1)."""
    res = []
    for k, desc in enumerate(descs):
        for rec in run_program(desc, images, rows, dtype, adapter_tables, kind=None if len(descs) == 1 else k, sel=sel, dev=dev):
            res.append(dict(rec, prog=k))
    return res


def stored_rows(rec, dst=None):
    """What the launch left at the rows a result covers: [R, C] of rec['dst'] (or of `dst`, a tensor of the same geometry)."""
    t = rec["dst"] if dst is None else dst
    return t[..., :C][rec["img"].to(t.device) // rec["div"], rec["row"].to(t.device)]


def as_images(x, rows):
    """[R, C] of whole images, image-major -> [images, rows, C] (the shape launch_shadow.compare tiles)."""
    return x.reshape(-1, rows, x.shape[-1])
