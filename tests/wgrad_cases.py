"""Case table of cgen_conv2d_wgrad's generic kernel (wgrad_kernel<T, NTC>, kind 0) and tiled kernel (wgrad_tile_kernel<NCF, NJW, KS>,
kind 1) of csrc/wgrad.hip, and a plain-Python mirror of the host-side dispatch: wg3_plan (csrc/wgrad3.hip; which shapes the streaming
kernel takes, kinds 2 / 3, and with how many splits), wgrad_tiled_ok / wgrad2_geometry and wgrad_geometry / wgrad_ntc / vec16_ok, all at
the default knobs.  `record()` returns what cgen_conv2d_wgrad_plan_record must answer.  Shared by tests/test_gpu_wgrad_f64.py (runs every
case against the f64 reference of tests/wgrad_ref.py) and tests/test_wgrad_cases.py (holds the mirror to the built library without a GPU
and checks that the table reaches every instance and boundary).

A view of `c` channels lies in a parent [n + 1, step h + 1, step w + 1, pc] at channel offset `off`, every `step`-th pixel of it (the
ResNet's strided "even" view); a stride-0 view (`bcast`) in [n + 1, 1, 1, pc].  The parent is allocated whole, 256-byte aligned, so the
view's alignment is off * esz.  Channels [c, cpad) hold zeros, everything else around the view NaN.

Only CGEN_WGRAD_GENERIC is used of the knobs (`generic`): wgrad_tiled_ok reads it on every call.  Everything the library caches in a
function-local static stays at its default; what that leaves out is listed under LABNOTES 38."""
from dataclasses import dataclass

NONE, RELU, GELU = 0, 1, 2
MAC_CAP = 10 ** 9  # (tests/conv_cases.py's)
TILE_H, TILE_W, WG_PK, WG_MAXT, WG2_MAXACC = 8, 16, 64, 9, 24
W3_PN, W3_SN = 6, 3
REC_INTS = 24
KIND0_FIELDS = ("dtype", "ntc", "n_cichunks", "n_tapgroups", "pix_per_split", "gout_vec", "seg_vec", "bias")
KIND1_FIELDS = ("ncf", "njw", "ks", "cwin", "n_cwin", "n_co", "ntiles", "tps", "dbuf", "lds", "variant")


def _ceil_div(a, b):
    return -(-a // b)


def _pad(v, m):
    return _ceil_div(v, m) * m


@dataclass(frozen=True)
class V:
    """Where a view lies in its parent.  pc = 0: the narrowest multiple of 8 that leaves 8 channels after the view."""
    off: int = 8
    pc: int = 0
    cpad: int = 0
    bcast: bool = False
    step: int = 1

    def tag(self):
        return f"o{self.off}p{self.pc}" + (f"c{self.cpad}" if self.cpad else "") + ("b" if self.bcast else "") + (f"s{self.step}" if self.step > 1 else "")


AL = V()


def tight(c):
    return V(0, c)


def pad8(c):
    return V(8, 0, _pad(c, 8))


@dataclass(frozen=True)
class Case:
    dt: str  # "f32" or "h16" (the library's 16-bit format)
    n: int
    h: int
    w: int
    segs: tuple
    co: int
    ks: int
    act: int = NONE
    views: tuple = ()  # one V per segment; absent: AL
    gv: V = AL
    bias: bool = True
    accumulate: bool = False
    unscale: float = 1.0
    generic: bool = False  # CGEN_WGRAD_GENERIC=1
    want: str = ""  # the instance this case was written for (tag())
    note: str = ""

    @property
    def esz(self):
        return 4 if self.dt == "f32" else 2

    def v(self, s):
        return self.views[s] if s < len(self.views) else AL

    def macs(self):
        return self.n * self.h * self.w * self.ks * self.ks * sum(self.segs) * self.co

    def id(self):
        s = f"{self.dt}-{self.want}-n{self.n}x{self.h}x{self.w}-c{'+'.join(map(str, self.segs))}-o{self.co}-k{self.ks}-" + ("none", "relu", "gelu")[self.act]
        s += "-b" if self.bias else ""
        s += "-acc" if self.accumulate else ""
        s += "-us" if self.unscale != 1.0 else ""
        for k, vw in enumerate(self.views):
            if vw != AL:
                s += f"-s{k}:{vw.tag()}"
        if self.gv != AL:
            s += f"-g:{self.gv.tag()}"
        return s + ("-generic" if self.generic else "")


# ------------------------------------------------------------------------------------------------------------- layout
def parent_shape(case, c, vw):
    """(parent shape, parent channel width) of a view of `c` channels laid out by `vw`."""
    pc = vw.pc if vw.pc else _pad(vw.off + max(c, vw.cpad), 8) + 8
    assert pc >= vw.off + max(c, vw.cpad)
    if vw.bcast:
        return (case.n + 1, 1, 1, pc)
    return (case.n + 1, vw.step * case.h + 1, vw.step * case.w + 1, pc)


def view(case, c, vw):
    """The cgen_view as the library sees it: p = byte offset from a 256-byte aligned base."""
    _, ph, pw, pc = parent_shape(case, c, vw)
    if vw.bcast:
        return dict(p=vw.off * case.esz, sn=pc, sh=0, sw=0, c=c, cpad=vw.cpad)
    return dict(p=vw.off * case.esz, sn=ph * pw * pc, sh=vw.step * pw * pc, sw=vw.step * pc, c=c, cpad=vw.cpad)


def problem(case):
    """The call as the mirror takes it."""
    return dict(dt=case.dt, n=case.n, h=case.h, w=case.w, ks=case.ks, act=case.act, bias=case.bias, generic=case.generic,
                seg=[view(case, c, case.v(s)) for s, c in enumerate(case.segs)], gout=view(case, case.co, case.gv))


# ------------------------------------------------------------------------------------------------------------- the mirror
def vec16_ok(v, esz):
    return v["p"] % 16 == 0 and all((v[k] * esz) % 16 == 0 for k in ("sn", "sh", "sw"))


def dma_clean(v, esz):
    g = 16 // esz
    small = 0 <= v["sh"] < (1 << 24) and 0 <= v["sw"] and v["sw"] * 64 < (1 << 24)
    return vec16_ok(v, esz) and (v["c"] % g == 0 or v["cpad"] >= _pad(v["c"], g)) and small


def _w3_op(sp, rows, rowpx):
    gpp = sp // 16
    ppi = 64 // gpp
    npx = rows * rowpx
    ninstr = _ceil_div(npx, ppi)
    return dict(npx=npx, ninstr=ninstr, bytes=ninstr * ppi * sp)


def wg3_plan(q):
    """(layout, nsplit) of the streaming kernel, or None where wg3_plan declines (default knobs)."""
    n, h, w, ks = q["n"], q["h"], q["w"], q["ks"]
    if q["dt"] != "h16" or ks not in (1, 3, 7) or q["gout"]["c"] <= 0:
        return None
    views = [q["gout"]] + q["seg"]
    if not all(dma_clean(v, 2) for v in views):
        return None
    for v in views:
        ext = n * v["sn"] + (h + 34) * v["sh"] + (w + 34) * v["sw"] + v["c"] + 8
        if not (ext * 2 < (1 << 31) and v["sn"] >= 0):
            return None
    taps, co = ks * ks, q["gout"]["c"]
    cx8, ci_total = sum(_pad(v["c"], 8) for v in q["seg"]), sum(v["c"] for v in q["seg"])
    cg8 = _pad(co, 8)
    if co * taps * ci_total >= (1 << 29):
        return None
    x_is_s = cx8 <= cg8
    cs8, cp8 = (cx8, cg8) if x_is_s else (cg8, cx8)
    NS, MPT = _ceil_div(taps * cs8, 32), _ceil_div(cp8, 32)
    best = None
    for WM, WN, WK in ((1, 4, 1), (2, 2, 1), (4, 1, 1), (1, 2, 2), (2, 1, 2), (1, 1, 4)):
        for NSW in range(1, 5):
            if NSW > 1 and WN * (NSW - 1) >= NS:
                break
            mpw_max = 2 if NSW == 4 else (3 if NSW == 3 else 4)
            nswin = _ceil_div(NS, WN * NSW)
            nwin = _ceil_div(MPT, WM * mpw_max)
            MPW = _ceil_div(_ceil_div(MPT, nwin), WM)
            if WK > 1 and (4 // WK) * (MPW * NSW * 16 + max(MPW, NSW)) * 256 > 48 * 1024:
                continue
            nbytes = nswin * cp8 + nwin * nswin * cs8 * 2
            mfma = nwin * nswin * MPW * NSW * 12 // WK
            reads = nwin * nswin * (MPW + NSW) * 12 // WK
            key = (nbytes << 36) + (mfma << 18) + reads
            if best is None or key < best[0]:
                best = (key, WM, WN, WK, MPW, NSW)
    if best is None:
        return None
    _, WM, WN, WK, MPW, NSW = best
    pwin_c = MPW * WM * 32
    n_pwin, n_swin = _ceil_div(cp8, pwin_c), _ceil_div(NS, WN * NSW)
    wP = min(pwin_c, cp8)
    spP, spS = _pad(wP * 2, 16), _pad(cs8 * 2, 16)
    if spP in (256, 272):
        spP = 288
    if spP > 1024 or spS > 1024:
        return None
    halo = ks // 2
    pad16, pad8_ = _pad(w, 16), _pad(w, 8)
    tw = 8 if (w < 12 or pad8_ < pad16 or (pad8_ == pad16 and w % 16 != 0)) else 16
    kst_rows = 16 // tw
    hpad = _pad(h, kst_rows)
    pick = None
    for ps in range(3):
        bestc = 1e30
        for k, tpx in enumerate((512, 384, 256, 192, 128, 96, 64, 48, 32)):
            if tpx % tw:
                continue
            th = tpx // tw
            if th < kst_rows or th % kst_rows or th + 2 * halo > 60:
                continue
            if th > hpad and k != 8:
                continue
            P, S = _w3_op(spP, th, tw), _w3_op(spS, th + 2 * halo, tw + 2 * halo)
            slot = _pad(P["bytes"] + S["bytes"], 16)
            ns = min(3, 72 * 1024 // slot)
            fast = _ceil_div(P["ninstr"], 4) <= W3_PN and _ceil_div(S["ninstr"], 4) <= W3_SN
            counted = (_ceil_div(P["ninstr"], 4) + _ceil_div(S["ninstr"], 4)) * max(0, ns - 2) <= 15
            ok = (ns >= 3 and fast and counted) if ps == 0 else ((ns >= 2 and fast and counted) if ps == 1 else ns >= 2)
            if ok:
                kst = th * tw // 16
                cost = (_ceil_div(h, th) * th) / h * (kst + 2.5) / kst
                if cost < bestc - 1e-9:
                    bestc, pick = cost, tpx
        if pick is not None:
            break
    if pick is None:
        return None
    th = pick // tw
    S = _w3_op(spS, th + 2 * halo, tw + 2 * halo)
    ntiles = n * _ceil_div(w, tw) * _ceil_div(h, th)
    dbytes = 4 * co * taps * ci_total
    tile_bytes = 2 * (n_swin * th * tw * cp8 + n_pwin * n_swin * S["npx"] * cs8)
    blk = 2 * (th * tw * wP + S["npx"] * cs8)
    tps = max(1, 1536 * 1024 // blk)
    tps = max(tps, (2 * dbytes * 100 + 30 * tile_bytes - 1) // (30 * tile_bytes), 4)
    tps = min(tps, ntiles)
    return (0 if x_is_s else 1), _ceil_div(ntiles, tps)


def _pixtile(width, rows, npx):
    gpr = (width * 2 + 15) // 16 + 1
    if gpr % 2 == 0:
        gpr += 1
    ppp = 64 // gpr
    if ppp < 1:
        return dict(ppp=0, bytes=0)
    return dict(ppp=ppp, bytes=rows * _ceil_div(npx, ppp) * 1024)


def wgrad2_geometry(N, H, W, co, ctot8, ks):
    if ks not in (1, 3, 7) or H < 1 or W < 1:
        return None
    taps, halo = ks * ks, ks // 2
    ncf = 1 if co <= 16 else (2 if co <= 32 else (4 if co <= 64 else (6 if co <= 96 else 8)))
    njw = 16 if ncf == 1 else WG2_MAXACC // ncf
    c16 = _pad(ctot8, 16)
    HH, HW = TILE_H + 2 * halo, TILE_W + 2 * halo
    if ks != 7:
        co8 = _pad(co, 8)
        best = base = -1
        bncf, bnjw = ncf, njw
        for cf, jw in ((1, 16), (2, 12), (2, 16), (4, 6), (6, 4), (8, 3)):
            if cf > ncf:
                continue
            mg = 4 * jw // taps
            if mg < 1:
                continue
            cw = min(mg * 16, c16)
            gt = _pixtile(cf * 16, TILE_H, TILE_W)
            while cw >= 16:
                xt = _pixtile(cw, HH, HW)
                if gt["ppp"] >= 1 and xt["ppp"] >= 1 and xt["bytes"] + gt["bytes"] <= 78 * 1024:
                    break
                cw -= 16
            if cw < 16:
                continue
            nbytes = _ceil_div(co, cf * 16) * _ceil_div(ctot8, cw) * (HH * HW * min(cw, ctot8) * 2 + TILE_H * TILE_W * min(cf * 16, co8) * 2)
            if cf == ncf and jw == njw:
                base = nbytes
            if best < 0 or nbytes < best:
                best, bncf, bnjw = nbytes, cf, jw
        if base > 0 and (bncf, bnjw) != (ncf, njw) and best * 100 <= base * 90:
            ncf, njw = bncf, bnjw
    else:
        if ctot8 > 16:
            return None
        ncf, njw = (1 if co <= 16 else 2), 16
    maxgrp = 4 * njw // taps
    if maxgrp < 1:
        return None
    cwin = min(maxgrp * 16, c16)
    gt = _pixtile(ncf * 16, TILE_H, TILE_W)
    while True:
        if cwin < 16:
            return None
        xt = _pixtile(cwin, HH, HW)
        if gt["ppp"] >= 1 and xt["ppp"] >= 1 and xt["bytes"] + gt["bytes"] <= 78 * 1024:
            break
        cwin -= 16
    lds = xt["bytes"] + gt["bytes"]
    dbuf = 1 if 2 * lds <= 78 * 1024 else 0
    if dbuf:
        lds *= 2
    n_cwin, n_co = _ceil_div(ctot8, cwin), _ceil_div(co, ncf * 16)
    ntiles = N * _ceil_div(W, TILE_W) * _ceil_div(H, TILE_H)
    want = _ceil_div(32, n_cwin * n_co)
    wbytes = 4 * co * taps * ctot8
    want = max(1, min(want, (4096 << 20) // max(wbytes, 1)))
    tps = _ceil_div(ntiles, want)
    min_tps = 16 if N <= 64 else 4
    if tps < min_tps and ntiles >= min_tps:
        tps = min_tps
    variant = 32 + ncf if ks == 7 else ((36 + (ks == 3)) if (ncf == 2 and njw == 16) else ncf * 2 + (ks == 3))
    return dict(ncf=ncf, njw=njw, ks=ks, cwin=cwin, n_cwin=n_cwin, n_co=n_co, ntiles=ntiles, tps=tps, dbuf=dbuf, lds=lds, variant=int(variant),
                nsplit=_ceil_div(ntiles, tps))


def wgrad_tiled(q):
    if q["dt"] != "h16" or q["generic"]:
        return None
    views = [q["gout"]] + q["seg"]
    if not all(dma_clean(v, 2) for v in views):
        return None
    for v in views:
        ext = q["n"] * v["sn"] + (q["h"] + TILE_H + q["ks"]) * v["sh"] + (q["w"] + TILE_W + q["ks"]) * v["sw"] + v["c"]
        if not ext * 2 < (1 << 31):
            return None
    return wgrad2_geometry(q["n"], q["h"], q["w"], q["gout"]["c"], sum(_pad(v["c"], 8) for v in q["seg"]), q["ks"])


def wgrad_ntc(co):
    return 1 if co <= 16 else (2 if co <= 32 else 4)


def wgrad_geometry(P, co, ci_chunks, ks):
    tiles = ci_chunks * _ceil_div(co, wgrad_ntc(co) * 16) * _ceil_div(ks * ks, WG_MAXT)
    nsplit = max(1, min(_ceil_div(2048, tiles), _ceil_div(P, 4 * WG_PK)))
    pps = _pad(_ceil_div(P, nsplit), WG_PK)
    return _ceil_div(P, pps), pps


def plan(q):
    """dict(kind, nsplit, ...the fields of the kind by name)."""
    g3 = wg3_plan(q)
    if g3 is not None:
        return dict(kind=2 + g3[0], nsplit=g3[1])
    g2 = wgrad_tiled(q)
    if g2 is not None:
        return dict(kind=1, **g2)
    esz = 4 if q["dt"] == "f32" else 2
    co, ks = q["gout"]["c"], q["ks"]
    chunks = sum(_ceil_div(v["c"], 32) for v in q["seg"])
    ci_total = sum(v["c"] for v in q["seg"])
    nsplit, pps = wgrad_geometry(q["n"] * q["h"] * q["w"], co, _ceil_div(ci_total, 32), ks)
    g, al = q["gout"], 4 * esz
    return dict(kind=0, nsplit=nsplit, dtype=0 if q["dt"] == "f32" else 1, ntc=wgrad_ntc(co), n_cichunks=chunks, n_tapgroups=_ceil_div(ks * ks, WG_MAXT),
                pix_per_split=pps, gout_vec=int(g["p"] % al == 0 and all((g[k] * esz) % al == 0 for k in ("sn", "sh", "sw"))),
                seg_vec=sum(int(vec16_ok(v, esz)) << s for s, v in enumerate(q["seg"])), bias=int(q["bias"]))


def record(q):
    """cgen_conv2d_wgrad_plan_record's out[0 .. 23]."""
    p = plan(q)
    names = KIND0_FIELDS if p["kind"] == 0 else (KIND1_FIELDS if p["kind"] == 1 else ())
    rec = [p["kind"], p["nsplit"]] + [p[k] for k in names]
    return rec + [0] * (REC_INTS - len(rec))


def tag(p):
    if p["kind"] == 0:
        return f"gen-ntc{p['ntc']}-tg{p['n_tapgroups']}"
    if p["kind"] == 1:
        return f"tile-{p['ncf']}-{p['njw']}-{p['ks']}"
    return f"stream{p['kind']}"


# ------------------------------------------------------------------------------------------------------------- the table
def _c(dt, n, h, w, segs, co, ks, act=NONE, want="", **kw):
    return Case(dt, n, h, w, tuple(segs), co, ks, act, want=want, **kw)


US = 2.0 ** -10  # (the f16 engine's loss scales are powers of two: the product with the sum is exact)
RN = dict(bias=False)  # the ResNet's conv sites have no conv bias: ChestPredictorTrainStep passes partial_b = NULL


def _gen_cases(dt):
    """Kind 0 in one element type.  Views are chosen so that the streaming and tiled kernels decline a 16-bit call: a channel count that
    is no multiple of 8 with cpad = 0, or 5 x 5, unless the case says otherwise."""
    h16 = dt == "h16"
    u = tight if not h16 else (lambda c: V(8, 0, 0))  # f32: the view is its parent; h16: aligned, unpadded
    out = [
        # ragged everything: P = 126 is one full and one 62-pixel K-step; Co = 3 in a 3-wide parent (gout_vec off), 5 channels in a
        # 5-wide parent (f32: the row stride is no multiple of 16 bytes, seg_vec off)
        _c(dt, 2, 9, 7, [5], 3, 3, RELU, "gen-ntc1-tg1", views=(tight(5),), gv=tight(3), note="ragged everything"),
        # split-K with a ragged last split: 192 + 138 pixels, the last K-step has 10
        _c(dt, 3, 10, 11, [5 if h16 else 8], 8, 3, RELU, "gen-ntc1-tg1", note="two splits, ragged last"),
        # Co classes
        _c(dt, 2, 5, 6, [40], 24, 5 if h16 else 3, GELU, "gen-ntc2-tg3" if h16 else "gen-ntc2-tg1", note="Co 17..32; chunks 32 + 8"),
        _c(dt, 1, 6, 6, [48, 20], 33, 5 if h16 else 1, NONE, "gen-ntc4-tg3" if h16 else "gen-ntc4-tg1", note="one ragged 64-wide co tile; seg_off"),
        _c(dt, 2, 4, 5, [24, 4, 40], 100, 5 if h16 else 3, RELU, "gen-ntc4-tg3" if h16 else "gen-ntc4-tg1", views=(AL, V(8, 0, 0, True), AL),
           note="two co tiles (64 + 36) with a bias; the parents as a stride-0 segment", accumulate=True, unscale=US),
        # a segment's vector path with a scalar tail, and the same shape without the vector path
        _c(dt, 2, 5, 5, [13 if h16 else 5], 8, 3, GELU, "gen-ntc1-tg1", views=(V(8, 0, 0),), note="seg_vec on, scalar tail"),
        _c(dt, 2, 5, 5, [13 if h16 else 5], 8, 3, GELU, "gen-ntc1-tg1", views=(V(1, 0, 0) if h16 else tight(5),), note="seg_vec off"),
        # grad_out at an odd channel offset
        _c(dt, 2, 5, 5, [13 if h16 else 8], 12, 3, NONE, "gen-ntc1-tg1", views=(u(13),), gv=V(3), note="gout_vec off: slice at an odd offset"),
        # 5 x 5: three tap groups of 9 / 9 / 7; 7 x 7: six, the last with 4 taps
        _c(dt, 2, 6, 6, [8], 16, 5, RELU, "gen-ntc1-tg3", note="5x5 (16-bit: dma_clean views, the vector path)"),
        _c(dt, 2, 20, 20, [1], 16, 7, NONE, "gen-ntc1-tg6", views=(u(1),), note="the stem"),
        _c(dt, 2, 6, 6, [3], 32, 7, NONE, "gen-ntc2-tg6", views=(u(3),)),
        # images smaller than the kernel
        _c(dt, 4, 1, 1, [130], 70, 3, GELU, "gen-ntc4-tg1", views=(u(130),), note="eight of nine taps are zeros over the NaN prefill"),
        _c(dt, 3, 2, 2, [16 if not h16 else 12], 16, 3, RELU, "gen-ntc1-tg1", views=(u(16 if not h16 else 12),)),
        _c(dt, 1, 3, 2, [8 if not h16 else 4], 8, 7, NONE, "gen-ntc1-tg6", views=(u(8 if not h16 else 4),), accumulate=True),
    ]
    return out


CASES = _gen_cases("f32") + [
    # ResNet-18's own calls at N = 2 (csrc/predictor_resnet_train.inc): f32, no activation, no bias partial
    _c("f32", 2, 7, 7, [512], 512, 3, NONE, "gen-ntc4-tg1", views=(tight(512),), gv=tight(512), note="layer4 3x3", **RN),
    _c("f32", 2, 7, 7, [4608], 512, 1, NONE, "gen-ntc4-tg1", views=(tight(4608),), gv=tight(512), note="a strided 3x3 as im2col: 144 chunks", **RN),
    _c("f32", 2, 12, 12, [49], 64, 1, NONE, "gen-ntc4-tg1", views=(V(0, 56, 56),), gv=tight(64), note="the stem as im2col, c 49 in cpad 56", **RN),
    _c("f32", 2, 4, 4, [64], 128, 1, NONE, "gen-ntc4-tg1", views=(V(0, 64, 0, False, 2),), gv=tight(128), note="1x1 downsample over the even view", **RN),
] + _gen_cases("h16") + [
    # (the streaming kernel takes most 7x7 calls on dma_clean views whatever their width; 24 -> 100 is one it declines, and the tiled kernel
    # has no 7x7 form beyond 16 input channels)
    _c("h16", 1, 5, 6, [24], 100, 7, RELU, "gen-ntc4-tg6", note="7x7 with 24 input channels, dma_clean views"),
    _c("h16", 2, 5, 5, [16], 8, 3, GELU, "gen-ntc1-tg1", views=(V(1),), gv=V(1), note="every base 2 bytes past 16-byte alignment"),
]

_TILE3 = [
    (2, 6, 6, [256], 256, {}, "the smallest"),
    (2, 6, 6, [256], 264, {}, "a fifth co block, 8 wide"),
    (2, 6, 6, [264], 256, {}, "a ninth window with cw = 8"),
    (2, 6, 6, [256, 4, 256], 256, dict(views=(AL, V(8, 0, 8, True), AL)), "segment borders at 256 and 264 inside the windows; stride-0 parents"),
    (1, 9, 17, [256], 256, {}, "2 x 2 ragged tiles"),
    (3, 8, 16, [256], 256, dict(accumulate=True, unscale=US), "one whole tile per image"),
]
_TILE1 = [
    (2, 6, 6, [520], 520, {}, "last window 72 wide, last co block 40 of 96"),
    (1, 17, 9, [520], 528, dict(accumulate=True), "two splits, the last of one tile"),
]
for _generic in (False, True):
    for _k, (_n, _h, _w, _segs, _co, _kw, _note) in enumerate(_TILE3):
        _want = "gen-ntc4-tg1" if _generic else "tile-4-6-3"
        CASES.append(_c("h16", _n, _h, _w, _segs, _co, 3, (RELU, GELU, NONE)[_k % 3], _want, note=_note, generic=_generic, **_kw))
    for _k, (_n, _h, _w, _segs, _co, _kw, _note) in enumerate(_TILE1):
        _want = "gen-ntc4-tg1" if _generic else "tile-6-4-1"
        CASES.append(_c("h16", _n, _h, _w, _segs, _co, 1, (GELU, RELU)[_k % 2], _want, note=_note, generic=_generic, **_kw))
CASES += [
    # The co-block search of wgrad2_geometry (fewest bytes per tile position) trades the 64-wide block for a 32-wide one with a wider
    # window at some input widths: two more instances serve 3x3 layers at the default knobs.  <2, 16, 3>: windows of 112 channels, 328
    # = 112 + 112 + 104 (the last 16-group half padding), a ninth co block 8 wide; <2, 12, 3>: windows of 80, 360 = 4 x 80 + 40.
    _c("h16", 2, 6, 6, [328], 264, 3, RELU, "tile-2-16-3", note="ragged last window and co block"),
    _c("h16", 1, 9, 17, [328], 256, 3, GELU, "tile-2-16-3", note="2 x 2 ragged tiles"),
    _c("h16", 2, 6, 6, [208, 4, 112], 256, 3, NONE, "tile-2-16-3", views=(AL, V(8, 0, 8, True), AL), note="segment borders inside the windows"),
    _c("h16", 2, 6, 6, [360], 264, 3, RELU, "tile-2-12-3", note="ragged last window and co block"),
    _c("h16", 1, 9, 17, [360], 264, 3, GELU, "tile-2-12-3", accumulate=True, unscale=US),
    _c("h16", 2, 6, 6, [360], 264, 3, NONE, "tile-2-12-3", bias=False),
    # 1x1 beyond 560 channels: the streaming kernel declines every 1x1 whose narrower side exceeds 512 channels, and wgrad2_geometry starts
    # from the 128-wide co block for Co > 96.  <8, 3, 1>: windows of 64 channels, 568 = 8 x 64 + 56 (the last 16-group half padding), 584 =
    # 4 x 128 + 72; the ordinary wide layers 640 -> 640 and 1024 -> 1024 land here.  <4, 6, 1>: windows of 160, 584 = 3 x 160 + 104, 680 = 10 x 64 + 40.
    _c("h16", 2, 6, 6, [568], 584, 1, RELU, "tile-8-3-1", note="ragged last window and co block"),
    _c("h16", 1, 9, 17, [640], 640, 1, GELU, "tile-8-3-1", note="2 x 2 ragged tiles", accumulate=True, unscale=US),
    _c("h16", 2, 6, 6, [568], 584, 1, NONE, "tile-8-3-1", bias=False),
    _c("h16", 2, 6, 6, [1024], 1024, 1, RELU, "tile-8-3-1", note="1024 -> 1024"),
    _c("h16", 2, 6, 6, [320, 4, 256], 584, 1, GELU, "tile-8-3-1", views=(AL, V(8, 0, 8, True), AL), note="segment borders inside the windows"),
    _c("h16", 2, 6, 6, [584], 680, 1, RELU, "tile-4-6-1", note="ragged last window and co block"),
    _c("h16", 1, 9, 17, [584], 680, 1, GELU, "tile-4-6-1", note="2 x 2 ragged tiles"),
    _c("h16", 2, 6, 6, [584], 680, 1, NONE, "tile-4-6-1", bias=False),
    # every activation on the two instances of the square layers
    _c("h16", 2, 6, 6, [256], 256, 3, GELU, "tile-4-6-3", bias=False),
    _c("h16", 2, 6, 6, [256], 256, 3, NONE, "tile-4-6-3"),
    _c("h16", 2, 6, 6, [520], 520, 1, NONE, "tile-6-4-1"),
    _c("h16", 2, 6, 6, [520], 520, 1, RELU, "tile-6-4-1", bias=False),
]


def family(case):
    p = plan(problem(case))
    return "h16-tile" if p["kind"] == 1 else f"{case.dt}-gen"
