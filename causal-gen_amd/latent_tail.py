"""The latent tail of a decoder layer (a mixin of `Engine`): what follows the layer's prior and posterior Blocks -- reparam + KL, the 1x1
conv z_proj over [z | pa] (the new trunk) and the 1x1 conv z_feat_proj over [z | p_feat] (the next layer's prior input) -- as ONE
launch each way (csrc/latent_tail.hip: cgen_latent_tail_fwd / cgen_latent_tail_bwd; f16 only), with the bits and the tape entries of
the launches it stands for.  DESIGN.md 3.4; LABNOTES 18 (backward), 21 (forward), 28 (deterministic layers).

A layer has one of two forms, and the form is DATA here -- one forward, one backward, one recogniser:

  stochastic     z is drawn from q; q_loc / q_ls / a reparam tape entry in front of z_proj carry the posterior side
  deterministic  z = p_loc (the layers above z_max_res): q_loc and q_ls are None, no reparam entry; the same two entry points with
                 q_loc / q_ls absent

Where the two differ, and why (each is decided at the line that carries its letter):

  (a) knobs.  The stochastic forward honours lat_tail_fwd and the pixel floor lat_tail_fwd_minpx, the stochastic backward lat_tail_minpx;
      the deterministic form honours lat_tail_det alone, both ways, and has no pixel floor: its layers are the largest tensors of the
      model, where no floor was ever wanted (kept as found; both floors default to 0, no size class measured slower).  The backward of
      either form also needs lat_tail (asked in Engine.backward()).
  (b) absent views.  Deterministic: q_loc, q_ls, p_ls, eps, z (forward) and gz_in, q_loc, q_ls, p_loc, p_ls, z, out_q (backward) are
      NULL_VIEW -- that absence IS how the kernel is told the form (no struct field).  Stochastic: only eps may be NULL
      (the kernel draws from Philox then).  coef, coef_stride, logt, chan_scale, kl_*, rng and stream_id are set for the stochastic
      form only; the other form leaves the struct's zeros.
  (c) forward order after the commit.  Stochastic: new(z), kl_channel_sums if free bits are on (a launch of its own, counted), new(h'),
      new(zf), launch.  Deterministic: new(h'), new(zf), launch.  The order fixes the arena addresses, and with them what a captured
      graph replays: it is the order of the separate launches.
  (d) tape.  Stochastic: reparam, z_proj (tag _bw_tag), z_feat_proj into `tape_hold` with tag 0.  Deterministic: z_proj (tag _bw_tag),
      z_feat_proj into `tape_hold` with tag _bw_tag.  backward() ignores the tag (Engine.__init__), so the difference is dead; kept as
      found, this module changes no tape.
  (e) backward target.  The stochastic kernel may accumulate (acc_p / acc_q from grad_write), so only a frozen buffer or a pending
      rider on either base declines it.  The deterministic kernels do not accumulate (the whole 2Z + C pixel leaves in
      16-byte stores): they also decline once grad(pout) holds any interval of [0, 2Z + C).
  (f) counters.  lat_tails_fwd / lat_tails against lat_tails_det_fwd / lat_tails_det.

Both forms share every other gate: f16, no profiled step, no CGEN_ABLATE, no remainder plane on h / p_feat, no remainder trunk."""
import ctypes as C
import os

from . import _lib
from ._lib import ACT_NONE, F16, NULL_VIEW, View


class LatentTailMixin:
    def _init_latent_tail(self):
        # A stochastic decoder layer's backward latent tail -- the 1x1 data gradients of z_feat_proj and z_proj and the reparam backward,
        # three adjacent tape entries -- as ONE launch (cgen_latent_tail_bwd; _latent_tail_at / _bw_latent_tail).  0: the four launches.
        self.lat_tail = os.environ.get("CGEN_LAT_TAIL", "1") != "0"
        self.lat_tail_minpx = int(os.environ.get("CGEN_LAT_TAIL_MINPX", "0"))  # layers with fewer pixels (n * h * w) keep the four launches
        # its arithmetic: by default the four launches' own, bit for bit (every GEMM summed and rounded to binary16 where they store
        # grad(z) / grad(p_feat)); 1: one f32 sum and one rounding per output -- closer to exact, and no longer the same bits
        self.lat_tail_exact = os.environ.get("CGEN_LAT_TAIL_EXACT", "0") != "0"
        self.lat_tails = 0  # fused launches of the last backward()
        # The same layer's FORWARD tail -- reparam + KL, z_proj, z_feat_proj -- as one launch (cgen_latent_tail_fwd; latent_tail_fwd below):
        # the three launches' bits, the three tape entries.  0: the three launches.
        self.lat_tail_fwd = os.environ.get("CGEN_LAT_TAIL_FWD", "1") != "0"
        self.lat_tail_fwd_minpx = int(os.environ.get("CGEN_LAT_TAIL_FWD_MINPX", "0"))  # layers with fewer pixels (n * h * w) keep the three launches
        self.lat_tails_fwd = 0  # fused forward launches since begin()
        # The DETERMINISTIC decoder layers (z = p_loc: the layers above z_max_res, the largest tensors of the model) the same way, both
        # directions (the same two entry points without q_loc / q_ls; the same three functions with q_loc / r None).  0: z_proj and
        # z_feat_proj as launches of their own, their data gradients, the residual's copy into grad(p_feat) and the zero fill of grad(p_ls).
        self.lat_tail_det = os.environ.get("CGEN_LAT_TAIL_DET", "1") != "0"
        self.lat_tails_det = 0      # fused launches of deterministic layers in the last backward()
        self.lat_tails_det_fwd = 0  # ... in forward passes since begin()

    # ------------------------------------------------------------------ forward
    def latent_tail_fwd(self, site_p, site_f, q_loc, q_ls, p_loc, p_ls, p_feat, h, pa, eps=None, stream_id=0, logt=0.0, kl_ptr=None, kl_stride=0,
                        fb=None, tape_hold=None):
        """[reparam_kl ->] conv(z_proj, [z, pa], res1=h, res2=p_feat, trunk=True) -> conv(z_feat_proj, [z, p_feat]) (`site_f` None: the
        layer has none) as ONE launch on the current stream, with the separate launches' bits and their tape entries in their places
        (z_feat_proj's goes to `tape_hold`).  `q_loc` None: a deterministic layer, z = p_loc, no reparam; q_ls,
        p_ls and the arguments from `eps` to `fb` are not looked at.  Returns (z, h', zf or None), or None -- nothing done, the caller runs the launches -- when the kernel does not serve
        the layer, when per-site timing is on, or under CGEN_ABLATE."""
        det = q_loc is None
        if not (self.lat_tail_det if det else self.lat_tail_fwd) or self.dt != F16 or self.prof is not None or self._ablate:  # (a)
            return None
        n, hh, ww, zd, c = p_loc.n, p_loc.h, p_loc.w, p_loc.c, site_p.co
        if not det and n * hh * ww < self.lat_tail_fwd_minpx:  # (a)
            return None
        if h.rem or p_feat.rem or (self.trunk_rem and max(hh, ww) <= self.trunk_maxres):
            return None
        if site_p.ks != 1 or list(site_p.seg_c) != [zd, pa.c] or (site_f is not None and (site_f.ks != 1 or list(site_f.seg_c) != [zd, c])):
            return None
        t = _lib.LatentTailFwdArgs()
        t.dtype, t.n, t.h, t.w, t.z_dim, t.c, t.ctx = self.dt, n, hh, ww, zd, c, pa.c
        t.p_loc, t.p_feat, t.h_in, t.pa = p_loc.cv(), p_feat.cv(), h.cv(), pa.cv()
        # (probe views for _supported(), which looks at shapes, strides and alignment: the layout new() will give the outputs, at a
        # pointer with the arena's alignment)
        probe = lambda c_: View(h.base.ptr, hh * ww * c_, ww * c_, c_, c_, 0)
        t.h_out, t.zf = probe(c), (NULL_VIEW if site_f is None else probe(site_f.co))
        t.img_p, t.img_f = site_p.img_fwd, (site_f.img_fwd if site_f is not None else None)
        bp, bf = site_p.conv.bias, (site_f.conv.bias if site_f is not None else None)
        t.bias_p, t.bias_f = (bp.data_ptr() if bp is not None else None), (bf.data_ptr() if bf is not None else None)
        if det:  # (b)
            t.q_loc = t.q_ls = t.p_ls = t.eps = t.z = NULL_VIEW
        else:
            t.kl_stride, t.stream_id, t.logt = kl_stride, stream_id, logt
            t.q_loc, t.q_ls, t.p_ls, t.z = q_loc.cv(), q_ls.cv(), p_ls.cv(), probe(zd)
            t.eps = eps.cv() if eps is not None else NULL_VIEW
            t.rng, t.kl_part = self.rng_ptr(), kl_ptr
        if not self.lib.latent_tail_fwd_supported(C.byref(t)):
            return None
        # ---- committed: the allocations, the launches' bookkeeping and the tape entries of the separate calls, in their order (c)
        z = p_loc
        if not det:
            z = self.new(n, hh, ww, zd)
            t.z = z.cv()
            if fb is not None:
                self.lib.kl_channel_sums(self.dt, n, hh, ww, zd, q_loc.cv(), q_ls.cv(), p_loc.cv(), p_ls.cv(), logt, fb[0] + 4 * fb[2], fb[1], self.stream)
                self.launches += 1
        h2 = self.new(n, hh, ww, c)
        zf = self.new(n, hh, ww, site_f.co) if site_f is not None else None
        t.h_out, t.zf = h2.cv(), (zf.cv() if zf is not None else NULL_VIEW)
        self.lib.latent_tail_fwd(C.byref(t), self.stream)
        self.launches += 1
        if det:  # (f)
            self.lat_tails_det_fwd += 1
        else:
            self.lat_tails_fwd += 1
        if self.recording:  # (d)
            if not det:
                self.tape.append((self._bw_reparam, (q_loc, q_ls, p_loc, p_ls, z, logt, None if fb is None else fb[2], self.kl_coef_override)))
            if self._dbg_names is not None:
                self._dbg_names[id(h2.base)] = site_p.name
            self.tape.append((self._bw_conv, (site_p, [z, pa], ACT_NONE, h2, h, p_feat), self._bw_tag))
            if zf is not None:
                if self._dbg_names is not None:
                    self._dbg_names[id(zf.base)] = site_f.name
                (self.tape if tape_hold is None else tape_hold).append(
                    (self._bw_conv, (site_f, [z, p_feat], ACT_NONE, zf, None, None), self._bw_tag if det else 0))
        return z, h2, zf

    # ------------------------------------------------------------------ backward
    def _latent_tail_at(self, i):
        """tape[i], [i-1], [i-2] = z_feat_proj, z_proj, reparam of one decoder layer (backward order; a layer without z_feat_proj:
        tape[i], [i-1] = z_proj, reparam; a deterministic layer: no reparam entry): returns (f, a, r), their argument tuples -- f None
        for an absent z_feat_proj, r None for the deterministic form -- else None.  Recognised by structure alone: two 1x1 convs without
        activation that read z as their first segment, z_proj adding the channel slice [2Z, 2Z + C) of the prior Block's output (p_feat)
        as a residual, z_feat_proj reading that same slice as its second segment.  z is the reparam's z, drawn from slices of two
        bases; or, deterministic, the slice [0, Z) of the prior Block's output itself."""
        tape = self.tape

        def conv_at(j):
            if j < 0 or tape[j][0] != self._bw_conv:
                return None
            site, segs, act, out, r1, r2 = tape[j][1]
            return tape[j][1] if site.ks == 1 and act == ACT_NONE and len(segs) == 2 and segs[0].rg and site.seg_rg[0] else None

        a, f = conv_at(i), None
        if a is None:
            return None
        if a[4] is None and a[5] is None:  # no residuals: z_feat_proj, with z_proj behind it
            a, f, i = conv_at(i - 1), a, i - 1
            if a is None or f[1][0] is not a[1][0] or not (f[1][1].rg and f[0].seg_rg[1]):
                return None
        site, segs, _, out, r1, r2 = a
        zd = segs[0].c
        if i >= 1 and tape[i - 1][0] == self._bw_reparam:
            r = tape[i - 1][1]
            q_loc, q_ls, p_loc, p_ls, z = r[:5]
            if segs[0] is not z or not all(t.rg for t in (q_loc, q_ls, p_loc, p_ls)):
                return None
            pb, qb = p_loc.base, q_loc.base
            slices = ((q_loc, qb, 0), (q_ls, qb, zd), (p_loc, pb, 0), (p_ls, pb, zd))
            if pb is qb or any(t.base is not b or t.coff != o or t.c != zd for t, b, o in slices) or qb.c < 2 * zd:
                return None
        else:
            r, pb = None, segs[0].base
            if not self.lat_tail_det or segs[0] is pb or segs[0].coff != 0:  # (a)
                return None
        if (segs[1].rg and site.seg_rg[1]) or pb.c != 2 * zd + site.co:
            return None
        pf = [t for t in (r1, r2) if t is not None and t.base is pb]  # the residual that is p_feat
        if len(pf) != 1 or not pf[0].rg or pf[0].coff != 2 * zd or pf[0].c != site.co:
            return None
        if f is not None and (f[1][1].base is not pb or f[1][1].coff != 2 * zd or f[1][1].c != site.co):
            return None
        return f, a, r

    def _bw_latent_tail(self, f, a, r):
        """The entries _latent_tail_at found as one cgen_latent_tail_bwd launch.  Deterministic form (`r` None): the data gradients into
        grad(p_loc), grad(p_feat) with the residual's share, and zeros for grad(p_ls), which nobody writes -- the whole 2Z + C pixel of
        the prior Block's output gradient, so no copy is parked as a rider and no fill follows.  Returns False -- nothing done, the
        caller runs the separate launches -- when the kernel does not serve the shapes or a gradient buffer involved may not be written
        in place."""
        det = r is None
        site_z, segs_z, _, out_z, r1, r2 = a
        if det:
            z = p_loc = segs_z[0]
        else:
            q_loc, q_ls, p_loc, p_ls, z, logt, fb_col, coef_ptr = r
        zd, c = z.c, site_z.co
        if self._ablate or (not det and z.n * z.h * z.w < self.lat_tail_minpx):  # (a)
            return False
        targets = [p_loc.base.chan(0, 2 * zd + c)] + ([] if det else [q_loc.base.chan(0, 2 * zd)])
        if det:  # (e)
            e = self.grads.get(id(p_loc.base))
            if e is not None and self._missing(e[1], 0, 2 * zd + c) != [(0, 2 * zd + c)]:
                return False
        if any(self._frozen(v) or id(v.base) in self._riders for v in targets):
            return False
        g_h = self.grad_read(out_z)
        if g_h is None:
            return False
        g_f = self.grad_read(f[3]) if f is not None else None
        t = _lib.LatentTailArgs()
        t.dtype, t.n, t.h, t.w, t.z_dim, t.c = self.dt, z.n, z.h, z.w, zd, c
        t.parity = 0 if self.lat_tail_exact else 1
        t.g_h = g_h.cv()
        t.g_f = g_f.cv() if g_f is not None else NULL_VIEW
        if det:  # (b)
            t.gz_in = t.q_loc = t.q_ls = t.p_loc = t.p_ls = t.z = t.out_q = NULL_VIEW
        else:
            gz_in = self.grad_read(z)
            t.gz_in = gz_in.cv() if gz_in is not None else NULL_VIEW
            t.coef_stride, t.logt = 0, logt
            t.q_loc, t.q_ls, t.p_loc, t.p_ls, t.z = q_loc.cv(), q_ls.cv(), p_loc.cv(), p_ls.cv(), z.cv()
            t.coef = self.kl_coef_ptr if coef_ptr is None else coef_ptr
            t.chan_scale = None if fb_col is None else self.kl_chan_ptr + 4 * fb_col
        # (the views grad_write will hand out below: _gentry creates the buffers, as the separate launches' grad_write would)
        outs = [self._gentry(v.base)[0].chan(0, v.c).cv() for v in targets]
        t.out_p, t.out_q = outs[0], (NULL_VIEW if det else outs[1])
        if g_f is not None:
            t.img_fz, t.img_fp = f[0].img_dg[0], f[0].img_dg[1]
        t.img_pz = site_z.img_dg[0]
        if not self.lib.latent_tail_bwd_supported(C.byref(t)):
            return False
        # ---- committed: the bookkeeping of the entries, in their order
        if g_f is not None and self._needs_wgrad(f[0]):
            self._wgrad(f[0], f[1], ACT_NONE, g_f)
        for res in (r1, r2):
            if res is not None and res.rg and res.base is not p_loc.base:  # (p_feat's share of G_h is added by the kernel)
                self._grad_residual(res, g_h, out_z, segs_z)
        if self._needs_wgrad(site_z):
            self._wgrad(site_z, segs_z, ACT_NONE, g_h)
        gp, acc_p = self.grad_write(targets[0])
        t.out_p, t.acc_p = gp.cv(), 1 if acc_p else 0
        if det:  # (e), (f)
            assert not acc_p
            self.lat_tails_det += 1
        else:
            gq, acc_q = self.grad_write(targets[1])
            t.out_q, t.acc_q = gq.cv(), 1 if acc_q else 0
            self.lat_tails += 1
        self.lib.latent_tail_bwd(C.byref(t), self.stream)
        self.launches += 1
        return True
