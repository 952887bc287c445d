"""Case table of cgen_conv2d (csrc/conv.hip), forward and data gradient, and a plain-Python mirror of its host-side dispatch.  Shared by
tests/test_gpu_conv_f64.py (runs every case against the f64 references of tests/conv_ref.py and asks cgen_conv2d_last_kernel() which
kernel served it) and tests/test_conv_cases.py (checks, without a GPU, that the table reaches every arm, instance and boundary).

Every NHWC view of a case lies in a parent tensor [n + pn, h + ph, w + pw, off + max(c, cpad) + cext] at channel offset `off` (a Lay);
the parent is allocated whole (its base is at least 256-byte aligned), so the byte alignment of a view is `off * esz` and its strides are
those of the parent.  `arm()` mirrors conv_fill, smallp_takes, launch_conv and the decline conditions of launch_conv_px, launch_conv_ws
and launch_conv_tile; `plan()` also returns the instance (template arguments) the launch picks.

A data-gradient case describes the FORWARD conv (segment widths `segs`, `co` output channels) and the segment `k` whose gradient is asked
for: the kernel then sees ONE input segment of `co` channels (grad_out), `segs[k]` output channels and the weight image of
cgen_weight_prep mode 1 at seg_off = sum(segs[:k]); `act` is the dact of the epilogue (the forward activation, applied to `aux`).

Only the knobs conv.hip reads with getenv on every call are used (`force`): CGEN_CONV_GENERIC, CGEN_CONV_NO_PX, CGEN_CONV_NO_WS.  The
knobs it caches in a function-local static stay at their defaults, so these instances are NOT covered: conv_px_kernel with three or four
channel pairs (NP = 3, 4: CGEN_PX_MAXNP is 2) and whatever CGEN_PX_MINWG / CGEN_PX_LDS / CGEN_PX_MODE < 2 would select instead;
conv_ws_kernel on halo tiles above 100 KiB (CGEN_WS_MAXLDS) and its buckets 1 and 2 (declined: nkw < 3; CGEN_CONV_FORCE_WS does not
lift that); the small-image thresholds other than 6000 / 19000 / 60 (CGEN_SMALLP_*), and the by-side route switched off
(CGEN_CONV_NO_SMALLP).  conv_smallp_pair_kernel ("smlp2") belongs to cgen_conv2d_pair and is held bit for bit to two cgen_conv2d calls
by tests/test_gpu_ops.py."""
from dataclasses import dataclass, field

CONV_PT, TILE_H, TILE_W, PX_MAXKS = 128, 8, 16, 16
SMALLP_MAXP, SMALLP_MAXP_LONGK, SMALLP_LONGK = 6000, 19000, 60
PX_LDS_BUDGET, PX_MAX_NP, PX_MIN_WGS, WS_MAXLDS, TILE_BUDGET = 52 * 1024, 2, 512, 100 * 1024, 64 * 1024
WS_BUCKETS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)
WS_INSTANCES = (3, 4, 5, 6, 8, 10, 12, 16)
NONE, RELU, GELU = 0, 1, 2
MAC_CAP = 10 ** 9
FORCE_ENV = {None: (), "generic": ("CGEN_CONV_GENERIC",), "no_px": ("CGEN_CONV_NO_PX",), "no_px_no_ws": ("CGEN_CONV_NO_PX", "CGEN_CONV_NO_WS")}
ALL_FORCE_ENV = ("CGEN_CONV_GENERIC", "CGEN_CONV_NO_PX", "CGEN_CONV_NO_WS", "CGEN_CONV_FORCE_WS", "CGEN_TILE_DBG", "CGEN_WS_DBG")


@dataclass(frozen=True)
class Lay:
    """Where a view lies in its parent.  cext = -1: as many trailing parent channels (at least 8) as make the parent's width a multiple
    of 8, so that an aligned `off` gives a 16-byte aligned view."""
    off: int = 8
    cext: int = -1
    pn: int = 1
    ph: int = 1
    pw: int = 1
    cpad: int = 0

    def tag(self):
        return f"o{self.off}e{self.cext}p{self.pn}{self.ph}{self.pw}" + (f"c{self.cpad}" if self.cpad else "")


AL = Lay()  # the default: padded on every side, 16-byte aligned
TIGHT = Lay(0, 0, 0, 0, 0, 0)  # the view is its parent
ROLES = ("s0", "s1", "s2", "s3", "out", "aux", "res1", "res2")


@dataclass(frozen=True)
class Case:
    dir: str  # "fwd" or "dgrad"
    dt: str  # "f32", "h16" (the library's 16-bit format, cgen_h16_format()) or "f32s" (forward only)
    n: int
    h: int
    w: int
    segs: tuple  # widths of the forward conv's input segments
    co: int
    ks: int
    act: int = NONE  # forward: applied to the input; dgrad: the dact of the epilogue
    bias: bool = True
    res1: bool = False
    res2: bool = False
    res1_rem: bool = False
    out_rem: bool = False
    k: int = 0  # dgrad: the segment whose gradient is computed
    lay: tuple = field(default_factory=tuple)  # ((role, Lay), ...) -- roles of ROLES or "*"; absent: AL
    force: str = None
    want: str = ""  # the arm (and instance) this case was written for: "ws-n2-b10" ...; test_conv_cases.py holds plan() to it
    note: str = ""

    @property
    def esz(self):
        return 2 if self.dt == "h16" else 4

    @property
    def in_segs(self):
        """Widths of the segments the kernel reads."""
        return self.segs if self.dir == "fwd" else (self.co,)

    @property
    def out_c(self):
        return self.co if self.dir == "fwd" else self.segs[self.k]

    @property
    def seg_off(self):
        return sum(self.segs[:self.k])

    @property
    def has_aux(self):
        return self.dir == "dgrad" and self.act != NONE

    def layout(self, role):
        d = dict(self.lay)
        return d.get(role, d.get("*", AL))

    def present(self, role):
        if role.startswith("s"):
            return int(role[1:]) < len(self.in_segs)
        return {"out": True, "aux": self.has_aux, "res1": self.res1, "res2": self.res2}[role]

    def channels(self, role):
        return self.in_segs[int(role[1:])] if role.startswith("s") else self.out_c

    def L(self):
        """Real products per output."""
        return self.ks * self.ks * sum(self.in_segs)

    def macs(self):
        return self.n * self.h * self.w * self.L() * self.out_c

    def id(self):
        s = f"{self.dir}-{self.dt}-{plan_tag(self)}-n{self.n}x{self.h}x{self.w}-c{'+'.join(map(str, self.segs))}-o{self.co}-k{self.ks}"
        if self.dir == "dgrad":
            s += f"-seg{self.k}"
        s += "-" + ("none", "relu", "gelu")[self.act]
        s += "".join(t for t, on in (("-b", self.bias), ("-r1", self.res1), ("-r2", self.res2), ("-r1rem", self.res1_rem), ("-orem", self.out_rem)) if on)
        for role, l in self.lay:
            s += f"-{role}:{l.tag()}"
        if self.force:
            s += f"-{self.force}"
        return s


# ------------------------------------------------------------------------------------------------------------- layout
def parent_shape(case, role):
    """((pn, ph, pw, pc), channel offset, cpad) of the parent of view `role`."""
    l, c = case.layout(role), case.channels(role)
    cw = max(c, l.cpad)
    cext = l.cext if l.cext >= 0 else 8 + (-(l.off + cw)) % 8
    return (case.n + l.pn, case.h + l.ph, case.w + l.pw, l.off + cw + cext), l.off, l.cpad


def view(case, role):
    """The cgen_view of `role` as conv_fill sees it: dict(p = byte offset from a 256-byte aligned base, sn, sh, sw, c, cpad), or None."""
    if not case.present(role):
        return None
    (pn, ph, pw, pc), off, cpad = parent_shape(case, role)
    return dict(p=off * case.esz, sn=ph * pw * pc, sh=pw * pc, sw=pc, c=case.channels(role), cpad=cpad)


def rem_offset(case, role):
    """Byte offset of the remainder plane of `role` (out / res1): the plane is a second parent right behind the first."""
    (pn, ph, pw, pc), _, _ = parent_shape(case, role)
    return pn * ph * pw * pc * case.esz


# ------------------------------------------------------------------------------------------------------------- conv_shared.h / common.h
def ceil_div(a, b):
    return -(-a // b)


def pad_to(v, m):
    return ceil_div(v, m) * m


def vec16_ok(v, esz):
    return v is None or (v["p"] % 16 == 0 and all((v[s] * esz) % 16 == 0 for s in ("sn", "sh", "sw")))


def dma_clean(v, esz):
    G = 16 // esz
    small = 0 <= v["sh"] < 1 << 24 and 0 <= v["sw"] and v["sw"] * 64 < 1 << 24
    return vec16_ok(v, esz) and (v["c"] % G == 0 or v["cpad"] >= pad_to(v["c"], G)) and small


def fits_i32(v, n, h, w):
    return v is None or (n * v["sn"] + h * v["sh"] + w * v["sw"] + v["c"]) * 2 < 1 << 31


def lds_stride(width, esz):
    s = width + 8
    if ((s * esz // 16) & 1) == 0:
        s += 16 // esz
    return s


def mk_pixtile(width_elems, esz, rows, npx):
    gpr = (width_elems * esz + 15) // 16 + 1
    if gpr % 2 == 0:
        gpr += 1
    ppp = 64 // gpr
    if ppp < 1:
        return dict(gpr=gpr, ppp=0, ppr=0, rowbytes=0, bytes=0)
    ppr = ceil_div(npx, ppp)
    return dict(gpr=gpr, ppp=ppp, ppr=ppr, rowbytes=ppr * 1024, bytes=rows * ppr * 1024)


# ------------------------------------------------------------------------------------------------------------- conv_fill
def fill(case):
    esz = case.esz
    segs = [view(case, f"s{i}") for i in range(len(case.in_segs))]
    out, aux, res1, res2 = (view(case, r) for r in ("out", "aux", "res1", "res2"))
    taps = case.ks * case.ks
    p = dict(N=case.n, H=case.h, W=case.w, KS=case.ks, nseg=len(segs), Co=case.out_c, P=case.n * case.h * case.w, taps=taps, segs=segs,
             out=out, aux=aux, res1=res1, res2=res2, esz=esz, split=case.dt == "f32s")
    p["seg_vec"] = [vec16_ok(s, esz) for s in segs]
    p["ctot8"] = sum(pad_to(s["c"], 8) for s in segs)
    p["tap0"], p["tap1"] = (taps // 2, taps // 2 + 1) if (case.h == 1 and case.w == 1 and case.ks > 1) else (0, taps)
    p["dma_ok"] = all(dma_clean(s, esz) for s in segs)
    p["out_rem"], p["r1_rem"] = case.out_rem, case.res1 and case.res1_rem

    def epi_ok(v):
        return v is None or (v["p"] % (4 * esz) == 0 and all((v[s] * esz) % (4 * esz) == 0 for s in ("sn", "sh", "sw")))

    ep = (out, aux, res1, res2)  # (the bias is a tensor of its own: 16-byte aligned)
    p["epi_vec"] = all(epi_ok(v) for v in ep)
    p["epi_vec16"] = all(vec16_ok(v, esz) for v in ep)
    p["force_generic"] = case.force == "generic"
    p["no_px"] = case.force in ("no_px", "no_px_no_ws")
    p["no_ws"] = case.force == "no_px_no_ws"
    return p


def smallp_takes(p):
    nk = ceil_div(p["taps"] * p["ctot8"], 32)
    by_size = (p["P"] <= SMALLP_MAXP or (nk >= SMALLP_LONGK and p["P"] <= SMALLP_MAXP_LONGK)) and p["KS"] in (1, 3)
    by_side = (p["H"] < 5 or p["W"] < 5) and p["KS"] in (1, 3)
    if p["force_generic"] or not (by_size or by_side):
        return False
    if not all(p["seg_vec"]) or not all(fits_i32(s, p["N"], p["H"] + 2, p["W"] + 2) for s in p["segs"]):
        return False
    return p["dma_ok"]


def plan_smallp(p):
    """launch_conv_smallp (its own conditions repeat smallp_takes')."""
    return dict(arm="smlp", oneseg=p["nseg"] == 1, nks=ceil_div((p["tap1"] - p["tap0"]) * p["ctot8"], 32))


def _views_fit(p):
    return (all(fits_i32(s, p["N"], p["H"] + TILE_H + 2, p["W"] + TILE_W + 2) for s in p["segs"])
            and all(fits_i32(v, p["N"], p["H"] + TILE_H, p["W"] + TILE_W) for v in (p["out"], p["aux"], p["res1"], p["res2"])))


def px_lds(np_, nks, xt):
    ldw = lds_stride(nks * 32, 2)
    return ceil_div(np_ * 32 * (ldw // 8), 64) * 1024 + xt["bytes"]


def plan_px(p):
    halo = p["KS"] // 2
    nks = ceil_div(p["taps"] * p["ctot8"], 32)
    if nks > PX_MAXKS or not p["epi_vec16"]:
        return None
    Co = p["Co"]
    if Co % 8:
        c8 = pad_to(Co, 8)
        if Co % 4 or p["out"]["cpad"] < c8 or any(v is not None and v["cpad"] < c8 for v in (p["aux"], p["res1"], p["res2"])):
            return None
    if not _views_fit(p):
        return None
    xt = mk_pixtile(p["ctot8"], 2, TILE_H + 2 * halo, TILE_W + 2 * halo)
    if xt["ppp"] < 1:
        return None
    ntiles = p["N"] * ceil_div(p["W"], TILE_W) * ceil_div(p["H"], TILE_H)
    np_all = ceil_div(Co, 32)
    np_ = min(np_all, 4)
    while np_ > 1 and px_lds(np_, nks, xt) > PX_LDS_BUDGET:
        np_ -= 1
    if np_ == 3 and np_all == 4:
        np_ = 2
    rem = bool(p["out_rem"] or p["r1_rem"])
    if rem and np_ > 3:
        np_ = 3 if np_all % 3 == 0 else 2
    np_ = min(np_, PX_MAX_NP)
    while np_ > 1 and ntiles * ceil_div(np_all, np_) < PX_MIN_WGS:
        np_ -= 1
    if px_lds(np_, nks, xt) > 150 * 1024:
        return None
    return dict(arm="px", np=np_, oneseg=p["nseg"] == 1, rem=rem, ppp=xt["ppp"], nks=nks)


def plan_ws(p):
    halo = p["KS"] // 2
    nk = ceil_div(p["taps"] * p["ctot8"], 32)
    nkw = ceil_div(nk, 4)
    ntc = 1 if p["Co"] <= 16 else 2
    bk = next((b for b in WS_BUCKETS if b >= nkw), None)
    if bk is None:
        return None
    xt = mk_pixtile(p["ctot8"], 2, TILE_H + 2 * halo, TILE_W + 2 * halo)
    if xt["ppp"] < 1 or not p["epi_vec16"] or p["Co"] % 8:
        return None
    if not _views_fit(p):
        return None
    if max(xt["bytes"], 4 * ntc * TILE_H * 1024) > WS_MAXLDS:
        return None
    grid_y = ceil_div(p["Co"], ntc * 16)
    if nkw < 3 or nkw < 2 * grid_y:
        return None
    if bk not in WS_INSTANCES:
        return None
    return dict(arm="ws", ntc=ntc, bucket=bk, nkw=nkw, nk=nk, grid_y=grid_y, oneseg=p["nseg"] == 1)


def tile_lds(cw, taps, kstep, esz, wrows, hpx):
    G = 16 // esz
    kp = pad_to(taps * cw, kstep)
    ldc, ldw = lds_stride(cw, esz), lds_stride(kp, esz)
    return (ceil_div(wrows * (ldw // G), 64) + ceil_div(hpx * (ldc // G), 64)) * 1024


def plan_tile(p):
    esz, halo, taps = p["esz"], p["KS"] // 2, p["taps"]
    kstep = 16 if (esz == 4 and not p["split"]) else 32
    hpx = (TILE_H + 2 * halo) * (TILE_W + 2 * halo)
    ntiles = p["N"] * ceil_div(p["H"], TILE_H) * ceil_div(p["W"], TILE_W)
    Co = p["Co"]
    ntc = 1 if Co <= 16 else (2 if Co <= 32 else 4)
    if ntiles < 512 and ntc > 1:
        ntc = 1 if ntiles < 192 else 2
    cw = p["ctot8"]
    while True:
        if cw < 8:
            return None
        if tile_lds(cw, taps, kstep, esz, ntc * 16, hpx) <= TILE_BUDGET:
            break
        cw -= 8
    rem = esz == 2 and bool(p["out_rem"] or p["r1_rem"])
    return dict(arm="tile", ntc=ntc, cw=cw, windows=ceil_div(p["ctot8"], cw), rem=rem, split=p["split"], k=taps * cw, kstep=kstep, ntiles=ntiles)


def plan(case):
    """launch_conv: the arm and the instance that serve the case."""
    p = fill(case)
    fast = p["KS"] in (1, 3) and p["H"] >= 5 and p["W"] >= 5 and p["dma_ok"] and not p["force_generic"]
    if case.dt == "h16":
        if smallp_takes(p):
            return plan_smallp(p)
        if fast and not p["no_px"] and ceil_div(p["taps"] * p["ctot8"], 32) <= PX_MAXKS:  # (CGEN_PX_MODE 2: every short K)
            r = plan_px(p)
            if r:
                return r
        if fast and not p["no_ws"] and not p["out_rem"] and not p["r1_rem"]:
            r = plan_ws(p)
            if r:
                return r
    if fast:
        r = plan_tile(p)
        if r:
            return r
    Co = p["Co"]
    return dict(arm="gen", ntc=1 if Co <= 16 else (2 if Co <= 32 else 4), epi_vec=p["epi_vec"])


def arm(case):
    return plan(case)["arm"]


def plan_tag(case):
    r = plan(case)
    a = r["arm"]
    if a == "gen":
        return f"gen-n{r['ntc']}" + ("" if r["epi_vec"] else "s")
    if a == "tile":
        return f"tile-n{r['ntc']}-w{r['windows']}" + ("-rem" if r["rem"] else "") + ("-split" if r["split"] else "")
    if a == "px":
        return f"px-p{r['np']}-{'one' if r['oneseg'] else 'multi'}" + ("-rem" if r["rem"] else "") + f"-ppp{r['ppp']}-ks{r['nks']}"
    if a == "ws":
        return f"ws-n{r['ntc']}-b{r['bucket']}-{'one' if r['oneseg'] else 'multi'}"
    return f"smlp-{'one' if r['oneseg'] else 'multi'}-ks{r['nks']}"


def family(case):
    """The tolerance family: one measured k_acc each (tests/test_conv_cases.py)."""
    a = arm(case)
    return ("f32-" if case.dt != "h16" else "h16-") + a


# ----------------------------------------------------------------------------------------------------------------- the table
def _lay(**kw):
    return tuple(kw.items())


def _c(want, dir, dt, n, h, w, segs, co, ks, **kw):
    return Case(dir, dt, n, h, w, tuple(segs), co, ks, want=want, **kw)


def _generic_cases():
    cs = []
    for dt in ("f32", "h16"):
        g = dict(force="generic")
        # P on both sides of CONV_PT
        for w in (127, 128, 129):
            cs.append(_c("gen-n1", "fwd", dt, 1, 1, w, [8], 16, 3, act=RELU, **g))
        # Co on both sides of every NTC choice
        for co, t in ((16, "gen-n1"), (17, "gen-n2"), (32, "gen-n2"), (33, "gen-n4"), (64, "gen-n4"), (65, "gen-n4")):
            cs.append(_c(t, "fwd", dt, 2, 3, 5, [16], co, 3, res1=True, **g))
        # kernel sizes; 5 and 7 have no other kernel
        for ks in (1, 3, 5, 7):
            cs.append(_c("gen-n1", "fwd", dt, 2, 6, 7, [8], 12, ks, act=GELU if ks == 5 else NONE,
                         force="generic" if ks < 5 else None))
        # a 1x1 image: the centre tap only
        for ks in (3, 7):
            cs.append(_c("gen-n1", "fwd", dt, 5, 1, 1, [16], 8, ks, res2=True, force="generic" if ks == 3 else None))
        # ragged channels without cpad (not DMA-clean: no other kernel takes them), one to four segments, a 1-channel segment; K = 9 * 8 ..
        # is no multiple of 32
        for segs in ([5], [8, 1], [3, 16, 1], [8, 1, 5, 24]):
            cs.append(_c("gen-n2s", "fwd", dt, 2, 6, 7, segs, 20, 3, act=RELU, lay=_lay(out=Lay(off=1))))
        # an output / a residual misaligned for the 4-channel epilogue
        cs.append(_c("gen-n1s", "fwd", dt, 2, 6, 7, [8], 16, 3, res1=True, lay=_lay(res1=Lay(off=2 if dt == "h16" else 1)), **g))
        cs.append(_c("gen-n1", "fwd", dt, 2, 6, 7, [8], 16, 3, res1=True, res2=True, **g))
        # model shapes
        cs.append(_c("gen-n1", "fwd", dt, 2, 16, 16, [64], 16, 3, act=GELU, **g))
        cs.append(_c("gen-n2", "fwd", dt, 2, 8, 8, [32, 32], 32, 1, act=RELU, res1=True, **g))
        cs.append(_c("gen-n4", "fwd", dt, 3, 4, 4, [128], 128, 3, act=RELU, **g))
    # f32 on images with a side below 5: the tiled kernel does not take them
    cs.append(_c("gen-n1", "fwd", "f32", 2, 4, 9, [8], 16, 3))
    cs.append(_c("gen-n1", "fwd", "f32", 2, 9, 4, [8], 16, 3))
    cs.append(_c("gen-n1", "fwd", "f32", 2, 5, 4, [8], 16, 1, act=GELU))
    return cs


def _tile_cases():
    cs = []
    # ---- f32: image sizes around the 8 x 16 tile
    for (n, h, w) in ((1, 5, 5), (2, 8, 16), (1, 9, 17), (1, 16, 17), (1, 17, 16)):
        cs.append(_c("tile-n1-w1", "fwd", "f32", n, h, w, [8], 16, 3, act=RELU, res1=True))
    cs.append(_c("tile-n1-w1", "fwd", "f32", 2, 9, 17, [16], 8, 1, act=GELU))
    # every NTC choice: by Co, and reduced below 192 / 512 tiles
    cs.append(_c("tile-n1-w1", "fwd", "f32", 1, 8, 16 * 191, [8], 32, 1, note="191 tiles"))
    cs.append(_c("tile-n2-w1", "fwd", "f32", 1, 8, 16 * 192, [8], 32, 1, note="192 tiles"))
    cs.append(_c("tile-n2-w1", "fwd", "f32", 1, 8, 16 * 511, [8], 48, 1, note="511 tiles"))
    cs.append(_c("tile-n4-w1", "fwd", "f32", 1, 8, 16 * 512, [8], 48, 1, note="512 tiles"))
    cs.append(_c("tile-n1-w1", "fwd", "f32", 1, 8, 16 * 191, [8], 48, 1, note="191 tiles, Co > 32"))
    # K on both sides of a multiple of KSTEP = 16: 8, 16, 24 (1x1) and 72, 144 (3x3)
    for (segs, ks) in (([8], 1), ([16], 1), ([24], 1), ([16], 3), ([4, 8], 3)):
        cs.append(_c("tile-n1-w1", "fwd", "f32", 1, 9, 17, segs, 16, ks, res2=True))
    # more channels than one LDS window holds
    cs.append(_c("tile-n1-w2", "fwd", "f32", 1, 9, 17, [64], 16, 3, act=RELU))
    cs.append(_c("tile-n1-w4", "fwd", "f32", 1, 9, 17, [40, 64, 24], 16, 3))
    # ---- f32s (forward only)
    cs.append(_c("tile-n1-w1-split", "fwd", "f32s", 1, 9, 17, [16], 16, 3, act=RELU, res1=True))
    cs.append(_c("tile-n1-w1-split", "fwd", "f32s", 2, 8, 16, [8, 8], 24, 1, act=GELU))
    cs.append(_c("tile-n1-w2-split", "fwd", "f32s", 1, 9, 17, [72], 8, 3))
    cs.append(_c("tile-n2-w1-split", "fwd", "f32s", 1, 8, 16 * 192, [8], 32, 1, act=RELU, note="192 tiles"))
    cs.append(_c("tile-n4-w1-split", "fwd", "f32s", 1, 8, 16 * 512, [8], 48, 1, res1=True, note="512 tiles"))
    # ---- h16, by default: an output width conv_px / conv_ws cannot write in whole chunks, above the small-image limit
    cs.append(_c("tile-n1-w1", "fwd", "h16", 1, 78, 78, [8], 12, 1, act=RELU))
    cs.append(_c("tile-n1-w1", "fwd", "h16", 1, 77, 83, [16], 3, 3, res1=True))
    # remainder planes with more than 16 K-steps (conv_px has at most 16, conv_ws has no planes)
    cs.append(_c("tile-n1-w1-rem", "fwd", "h16", 1, 78, 78, [64], 8, 3, act=RELU, res1=True, res1_rem=True, out_rem=True))
    cs.append(_c("tile-n1-w1-rem", "fwd", "h16", 1, 77, 83, [64], 16, 3, act=GELU, res1=True, res2=True, out_rem=True))
    # ... and its NTC 2 / 4 instances: an output width conv_px cannot write in whole chunks, at 192 / 512 tiles
    cs.append(_c("tile-n2-w1-rem", "fwd", "h16", 4, 64, 96, [8], 20, 1, act=RELU, res1=True, res1_rem=True, out_rem=True, note="192 tiles"))
    cs.append(_c("tile-n4-w1-rem", "fwd", "h16", 8, 64, 128, [8], 36, 1, res1=True, res1_rem=True, out_rem=True, note="512 tiles"))
    # more than 64 K-steps (no conv_ws bucket) above the long-K small-image limit
    cs.append(_c("tile-n1-w3", "fwd", "h16", 1, 138, 138, [232], 8, 3, act=RELU))
    # through the knobs
    cs.append(_c("tile-n1-w1", "fwd", "h16", 1, 77, 83, [24], 16, 3, act=RELU, res1=True, force="no_px_no_ws"))
    cs.append(_c("tile-n2-w1", "fwd", "h16", 4, 64, 96, [8, 8], 32, 1, act=GELU, force="no_px_no_ws", note="192 tiles"))
    cs.append(_c("tile-n4-w1", "fwd", "h16", 8, 64, 128, [8], 40, 1, force="no_px_no_ws", note="512 tiles"))
    return cs


def _px_cases():
    cs = []
    B = (1, 78, 78)  # 6084 pixels: just above the small-image limit
    # ks 1 and 3; nks 1, 3, 7, 12, 14, 16 (ctot8 8, 24, 40, 56 against the 18-pixel tile row: 21, 12, 9, 7 pixels per piece)
    cs.append(_c("px-p1-one-ppp21-ks1", "fwd", "h16", *B, [8], 8, 1, act=RELU))
    cs.append(_c("px-p1-one-ppp21-ks3", "fwd", "h16", *B, [8], 32, 3, act=RELU, res1=True))
    cs.append(_c("px-p1-one-ppp12-ks7", "fwd", "h16", *B, [24], 40, 3, act=GELU))
    cs.append(_c("px-p1-multi-ppp9-ks12", "fwd", "h16", *B, [16, 24], 64, 3, res1=True, res2=True))
    cs.append(_c("px-p1-one-ppp7-ks16", "fwd", "h16", *B, [56], 8, 3, act=RELU))
    cs.append(_c("px-p1-one-ppp9-ks14", "fwd", "h16", *B, [48], 16, 3, res1=True))
    # 15 K-steps exist only as a 1x1 over 480 channels (a 3x3 has 14 or 16), whose one-pixel pieces exceed conv_px's 150 KiB of LDS
    # (128 KiB of pixels + 31 of weights); 240 channels are the last with two pixels per piece, 256 the first with one (145 KiB)
    cs.append(_c("px-p1-one-ppp2-ks8", "fwd", "h16", *B, [240], 8, 1, act=RELU))
    cs.append(_c("px-p1-one-ppp1-ks8", "fwd", "h16", *B, [256], 8, 1, res1=True))
    cs.append(_c("tile-n1-w3", "fwd", "h16", *B, [480], 8, 1, note="15 K-steps, 178 KiB"))
    cs.append(_c("tile-n1-w3", "fwd", "h16", *B, [544], 8, 1, note="17 K-steps: not conv_px; a 544-channel pixel exceeds a DMA piece: not conv_ws"))
    cs.append(_c("ws-n1-b5-one", "fwd", "h16", *B, [64], 8, 3, note="18 K-steps: not conv_px"))
    # several segments, one ragged with zero padding
    cs.append(_c("px-p1-multi-ppp12-ks7", "fwd", "h16", *B, [3, 8, 1], 16, 3, act=RELU, lay=_lay(s0=Lay(cpad=8), s2=Lay(cpad=8))))
    # Co % 8 == 4 with cpad on every epilogue operand
    cs.append(_c("px-p1-one-ppp21-ks3", "fwd", "h16", *B, [8], 12, 3, res1=True, res2=True,
                 lay=_lay(out=Lay(cpad=16), res1=Lay(cpad=16), res2=Lay(cpad=16))))
    cs.append(_c("tile-n1-w1", "fwd", "h16", *B, [8], 12, 3, res1=True, lay=_lay(out=Lay(cpad=16)), note="res1 without cpad: conv_px declines"))
    # remainder planes; with Co % 8 == 4, whose whole-chunk stores reach [Co, cpad) of both planes
    cs.append(_c("px-p1-one-rem-ppp21-ks3", "fwd", "h16", *B, [8], 12, 3, res1=True, res1_rem=True, out_rem=True,
                 lay=_lay(out=Lay(cpad=16), res1=Lay(cpad=16))))
    cs.append(_c("px-p1-one-rem-ppp21-ks3", "fwd", "h16", *B, [8], 32, 3, act=RELU, res1=True, res1_rem=True, out_rem=True))
    cs.append(_c("px-p1-multi-rem-ppp12-ks1", "fwd", "h16", *B, [16, 8], 16, 1, act=GELU, res1=True, out_rem=True))
    # enough tiles for two channel pairs per workgroup
    cs.append(_c("px-p2-one-ppp21-ks1", "fwd", "h16", 4, 64, 128, [8], 128, 1, act=RELU, note="256 tiles x 2 parts"))
    cs.append(_c("px-p2-one-ppp21-ks1", "fwd", "h16", 4, 64, 120, [8], 128, 1, note="256 tiles; a ragged last tile column"))
    cs.append(_c("px-p1-one-ppp21-ks1", "fwd", "h16", 4, 64, 112, [8], 128, 1, note="224 tiles x 2 parts < 512"))
    # a ragged image
    cs.append(_c("px-p1-one-ppp21-ks3", "fwd", "h16", 1, 77, 83, [8], 32, 3, act=RELU, res1=True))
    cs.append(_c("px-p1-one-ppp21-ks3", "fwd", "h16", 1, 17, 353, [8], 16, 3, note="6001 pixels: the first above the small-image limit"))
    return cs


def _ws_cases():
    cs = []
    B = (1, 78, 78)
    # one case per bucket reachable by default (more than 16 K-steps): nkw 5, 6, 7 (bucket 8, one padding K-step), 9, 11, 13
    for segs, co, tag in (([64], 16, "ws-n1-b5-one"), ([80], 32, "ws-n2-b6-one"), ([32, 64], 16, "ws-n1-b8-multi"), ([120], 32, "ws-n2-b10-one"),
                          ([152], 16, "ws-n1-b12-one"), ([176], 8, "ws-n1-b16-one")):
        cs.append(_c(tag, "fwd", "h16", *B, segs, co, 3, act=RELU, res1=len(segs) == 1))
    # nkw 16 (63 K-steps; 60 and more go to the small-image kernel up to 19000 pixels)
    cs.append(_c("ws-n1-b16-one", "fwd", "h16", 1, 138, 138, [224], 16, 3, act=RELU))
    # buckets 3 and 4
    cs.append(_c("ws-n1-b3-one", "fwd", "h16", *B, [32], 16, 3, act=GELU, force="no_px"))
    cs.append(_c("ws-n2-b4-multi", "fwd", "h16", *B, [40, 8], 24, 3, res1=True, res2=True, force="no_px"))
    # nkw on both sides of 2 * grid_y (Co = 96: three channel tiles)
    cs.append(_c("ws-n2-b6-one", "fwd", "h16", *B, [80], 96, 3))
    cs.append(_c("tile-n1-w1", "fwd", "h16", *B, [64], 96, 3, note="nkw 5 < 2 * 3: conv_ws declines"))
    # a ragged image.  (No 1x1 reaches conv_ws at the default knobs: up to 240 channels it has at most 8 K-steps -- nkw 2 -- and above
    # that one pixel per DMA piece makes the halo tile 128 KiB, over the 100 KiB limit)
    cs.append(_c("tile-n1-w2", "fwd", "h16", *B, [288], 16, 1, force="no_px", note="nkw 3, but 128 KiB of LDS: conv_ws declines"))
    cs.append(_c("ws-n1-b6-multi", "fwd", "h16", 1, 77, 83, [64, 16], 16, 3, act=RELU, res1=True))
    return cs


def _smallp_cases():
    cs = []
    # P around the 32-pixel workgroup and the 6000-pixel limit
    for (n, h, w) in ((1, 1, 31), (2, 4, 4), (1, 3, 11), (1, 60, 100)):
        cs.append(_c("smlp-one-ks3", "fwd", "h16", n, h, w, [8], 8, 3, act=RELU, res1=True))
    # the long-K limit: 59 / 60 K-steps at 19000 pixels, 60 at 19001
    cs.append(_c("tile", "fwd", "h16", 1, 100, 190, [1888], 8, 1, note="59 K-steps: not the small-image kernel"))
    cs.append(_c("smlp-one-ks60", "fwd", "h16", 1, 100, 190, [1920], 8, 1))
    cs.append(_c("tile", "fwd", "h16", 1, 31, 613, [1920], 8, 1, note="19003 pixels"))
    # a side below 5 at a large P; a 1x1 image (centre tap only: one K-step where nine taps have five)
    cs.append(_c("smlp-one-ks3", "fwd", "h16", 1, 4, 2000, [8], 8, 3, act=RELU))
    cs.append(_c("smlp-one-ks1", "fwd", "h16", 33, 1, 1, [16], 24, 3, res2=True))
    # nks 1, 3, 4, 5, 16, 17 (four waves, four K-steps in flight each)
    for segs, ks, nks in (([32], 1, 1), ([8], 3, 3), ([128], 1, 4), ([16], 3, 5), ([512], 1, 16), ([544], 1, 17)):
        cs.append(_c(f"smlp-one-ks{nks}", "fwd", "h16", 2, 7, 9, segs, 32, ks, act=GELU if nks == 5 else RELU))
    # Co 8, 24, 32, 40; several segments; remainder planes
    for co in (24, 40):
        cs.append(_c("smlp-multi-ks7", "fwd", "h16", 2, 7, 9, [8, 3, 1], co, 3, res1=True, lay=_lay(s1=Lay(cpad=8), s2=Lay(cpad=8))))
    cs.append(_c("smlp-one-ks5", "fwd", "h16", 2, 7, 9, [16], 32, 3, act=RELU, res1=True, res1_rem=True, out_rem=True))
    cs.append(_c("smlp-multi-ks2", "fwd", "h16", 2, 7, 9, [24, 24], 12, 1, act=GELU, res1=True, out_rem=True))
    return cs


def _dgrad_cases():
    cs = []
    D = dict(bias=False)
    # generic, both dtypes: every dact, with and without the accumulate; a segment at a non-zero seg_off
    for dt in ("f32", "h16"):
        for i, act in enumerate((NONE, RELU, GELU)):
            cs.append(_c("gen", "dgrad", dt, 2, 6, 7, [5, 12], 21, 3, act=act, res1=bool(i % 2), k=i % 2, **D))
        cs.append(_c("gen", "dgrad", dt, 2, 6, 7, [16], 24, 5, act=RELU, res1=True, **D))
        cs.append(_c("gen", "dgrad", dt, 5, 1, 1, [8, 16], 16, 3, act=GELU, k=1, force="generic", **D))
    # tile f32
    for i, act in enumerate((NONE, RELU, GELU)):
        cs.append(_c("tile", "dgrad", "f32", 1, 9, 17, [8, 16], 24, 3 if i else 1, act=act, res1=i != 1, k=i % 2, **D))
    cs.append(_c("tile-n1-w2", "dgrad", "f32", 1, 9, 17, [16], 64, 3, act=RELU, res1=True, **D))
    # tile h16
    cs.append(_c("tile", "dgrad", "h16", 1, 78, 78, [12, 8], 8, 3, act=RELU, res1=True, **D))
    cs.append(_c("tile", "dgrad", "h16", 1, 78, 78, [8, 12], 16, 1, act=NONE, k=1, **D))
    cs.append(_c("tile-n1-w1-rem", "dgrad", "h16", 1, 78, 78, [8], 64, 3, act=RELU, res1=True, res1_rem=True, out_rem=True, **D))
    cs.append(_c("tile", "dgrad", "h16", 1, 77, 83, [16, 8], 24, 3, act=GELU, res1=True, force="no_px_no_ws", **D))
    # px
    for i, act in enumerate((NONE, RELU, GELU)):
        cs.append(_c("px", "dgrad", "h16", 1, 78, 78, [8, 32], 8 if i else 24, 3, act=act, res1=i != 0, k=1, **D))
    cs.append(_c("px", "dgrad", "h16", 1, 77, 83, [64], 16, 1, act=GELU, **D))
    cs.append(_c("px-p1-one-rem-ppp21-ks3", "dgrad", "h16", 1, 78, 78, [16], 8, 3, act=RELU, res1=True, res1_rem=True, out_rem=True, **D))
    # ws
    for i, act in enumerate((NONE, RELU, GELU)):
        cs.append(_c("ws", "dgrad", "h16", 1, 78, 78, [16, 8], 64 + 16 * i, 3, act=act, res1=i != 2, k=i % 2, **D))
    cs.append(_c("ws-n2-b4-one", "dgrad", "h16", 1, 77, 83, [24], 48, 3, act=RELU, res1=True, force="no_px", **D))
    # smallp
    for i, act in enumerate((NONE, RELU, GELU)):
        cs.append(_c("smlp", "dgrad", "h16", 2, 7, 9, [8, 32], 16 + 16 * i, 3 if i != 1 else 1, act=act, res1=i != 0, k=1, **D))
    cs.append(_c("smlp-one-ks1", "dgrad", "h16", 33, 1, 1, [24], 16, 3, act=RELU, res1=True, **D))
    cs.append(_c("smlp", "dgrad", "h16", 1, 4, 2000, [8], 8, 3, act=GELU, res1=True, **D))
    return cs


GENERIC_CASES = _generic_cases()
TILE_CASES = _tile_cases()
PX_CASES = _px_cases()
WS_CASES = _ws_cases()
SMALLP_CASES = _smallp_cases()
DGRAD_CASES = _dgrad_cases()
CASES = GENERIC_CASES + TILE_CASES + PX_CASES + WS_CASES + SMALLP_CASES + DGRAD_CASES
