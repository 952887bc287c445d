"""Counterfactual parents on the GPU -- ``pgm.counterfactual(obs, do)`` followed by ``dscm.vae_preprocess`` as ONE launch
(csrc/pgm_cf.hip, ``cgen_pgm_counterfactual``): abduction, action and prediction over the mechanism records ``PgmTrainStep`` trains,
and the compact ``[B, ctx]`` parents the HVAE takes, factual and counterfactual.

``PgmCounterfactual.run`` works on device-resident tables (observations and intervention values share one column layout, rows are
picked by optional device index vectors, the intervened variables by a host list or a device mask word), writes into static
buffers and only enqueues, so it can sit inside ``torch.cuda.graph`` next to ``GraphedCounterfactual``.  ``DevicePGM`` is the
dict-in / dict-out face ``DSCM`` and ``CfEvaluator`` ask of a PGM.

Semantics (include/cgen_hip.h has the full statement): an intervened variable takes the ``do`` value bit for bit; a variable none
of whose ancestors is intervened on keeps the observation bit for bit (the host recomputes f(f^-1(obs)), which is the observation
up to rounding); every other conditional-affine variable is re-predicted from its abducted noise, and a Gumbel-max variable from
the posterior noise of its observed class.  A PGM the kernel does not serve raises ``ValueError``; nothing falls back to the host.
"""
import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from .dscm import _UKBB_LOG_STATS, _UKBB_MIN_MAX
from .pgm_train import build_records, default_columns


def touched(pgm, do_vars: Iterable[str]) -> List[str]:
    """The variables a counterfactual under ``do(do_vars)`` does not copy from the observation, in ``pgm.mechanisms()`` order: the
    intervened ones and everything downstream of them."""
    do, out = set(do_vars), []
    for m in pgm.mechanisms():
        if m.var in do or any(c in out for c in m.ctx):
            out.append(m.var)
    return out


def _widths(pgm) -> Dict[str, int]:
    return {m.var: (int(m.module.shape[-1]) if m.kind == "categorical" else 1) for m in pgm.mechanisms()}


def pre_records(pgm, args, columns: Dict[str, int], ncol: int) -> List[Tuple[int, int, int, float, float, float, float]]:
    """``vae_preprocess`` as data: one (col, width, kind, hi, lo, mu, sd) per entry of ``args.parents_x``.  With a ukbb data set
    every variable but ``sex`` and ``mri_seq`` is log-standardised with the constants of ``dscm.ukbb_preprocess``."""
    parents = list(getattr(args, "parents_x", None) or [])
    if not 1 <= len(parents) <= _lib.PGM_MAX_PRE:
        raise ValueError(f"PgmCounterfactual: {len(parents)} entries in args.parents_x, the kernel serves 1..{_lib.PGM_MAX_PRE}")
    ukbb = "ukbb" in (getattr(args, "dataset", "") or "")
    width, out = _widths(pgm), []
    for k in parents:
        if k not in columns:
            raise ValueError(f"PgmCounterfactual: no column was named for parent {k!r}")
        c0, w = int(columns[k]), width.get(k, 1)
        if not 0 <= c0 <= ncol - w:
            raise ValueError(f"PgmCounterfactual: parent {k!r}: columns {c0}..{c0 + w - 1} do not fit a table of {ncol} columns")
        if ukbb and k not in ("mri_seq", "sex"):
            if k not in _UKBB_MIN_MAX:
                raise ValueError(f"PgmCounterfactual: no ukbb range is known for parent {k!r}")
            (hi, lo), (mu, sd) = _UKBB_MIN_MAX[k], _UKBB_LOG_STATS[k]
            out.append((c0, w, _lib.PGM_PRE_LOGSTD, float(hi), float(lo), float(mu), float(sd)))
        else:
            out.append((c0, w, _lib.PGM_PRE_COPY, 0.0, 0.0, 0.0, 1.0))
    return out


class PgmCounterfactual:
    """The counterfactual launch of one PGM.  The records are built once from the parameters' addresses (in-place updates -- an
    optimiser step, ``load_state_dict``, ``PgmTrainStep``'s EMA model -- are picked up; moving the module to another device or
    dtype afterwards is not)."""

    def __init__(self, pgm, args=None, columns=None, ncol=None, exact_gumbel=None, device="cuda"):
        self.lib = _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if columns is None:
            columns, width = default_columns(pgm)
            ncol = width if ncol is None else ncol
        if ncol is None:
            raise ValueError("PgmCounterfactual: `ncol` (the table's width) is needed with named columns")
        self.columns, self.ncol = dict(columns), int(ncol)
        self.pgm = pgm.to(self.device)
        self.mechs = pgm.mechanisms()
        self.vars = [m.var for m in self.mechs]
        self.width = _widths(pgm)
        for i, m in enumerate(self.mechs):
            late = [c for c in m.ctx if c not in self.vars[:i]]
            if late:
                raise ValueError(f"PgmCounterfactual: mechanism {m.var!r} conditions on {late}, which no earlier mechanism produces "
                                 "(the kernel walks pgm.mechanisms() in order)")
        self.recs = build_records(pgm, self.columns, self.ncol)
        self.nmech = len(self.recs)
        self.gumbel = [i for i, m in enumerate(self.mechs) if m.kind == "gumbel_max"]
        self.exact_gumbel = bool(getattr(pgm, "exact_gumbel_posterior", False) if exact_gumbel is None else exact_gumbel)
        self.pre = pre_records(pgm, args, self.columns, self.ncol) if args is not None and getattr(args, "parents_x", None) else []
        self.ctx = sum(p[1] for p in self.pre)
        self._statics: Dict[int, dict] = {}

    # -- pieces -------------------------------------------------------------------------------------------
    def mask_of(self, do_vars: Iterable[str]) -> int:
        mask = 0
        for k in do_vars:
            if k not in self.vars:
                raise ValueError(f"PgmCounterfactual: cannot intervene on {k!r}: the PGM's variables are {self.vars}")
            mask |= 1 << self.vars.index(k)
        return mask

    def _entry(self, B: int) -> dict:
        ent = self._statics.get(B)
        if ent is None:
            dev = self.device
            ent = self._statics[B] = dict(
                cf=torch.zeros(B, self.ncol, device=dev), eps=torch.zeros(B, self.nmech, device=dev),
                pa=torch.zeros(B, self.ctx, device=dev) if self.pre else None, cf_pa=torch.zeros(B, self.ctx, device=dev) if self.pre else None,
                uniforms={i: torch.zeros(B, int(self.recs[i].ncls), device=dev) for i in self.gumbel})
        return ent

    def _table(self, t, what: str) -> Tensor:
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != self.ncol or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError(f"PgmCounterfactual.run: {what} must be a contiguous f32 [N, {self.ncol}] device tensor")
        return t

    @staticmethod
    def _index(idx, what: str):
        if idx is not None and (idx.dtype != torch.int64 or idx.dim() != 1 or idx.device.type != "cuda" or not idx.is_contiguous()):
            raise ValueError(f"PgmCounterfactual.run: {what} must be a device int64 vector")
        return idx

    # -- public -------------------------------------------------------------------------------------------
    def run(self, table: Tensor, index: Optional[Tensor] = None, do_table: Optional[Tensor] = None, do_index: Optional[Tensor] = None,
            do_vars: Optional[Sequence[str]] = None, do_mask_dev: Optional[Tensor] = None, uniforms=None, generator=None, rng: Optional[Tensor] = None):
        """Counterfactuals of rows ``index`` of ``table`` (all rows, in order, without an index) under ``do`` of the variables
        ``do_vars`` -- or of those whose bit (position in ``pgm.mechanisms()``) is set in the one-element int32 device tensor
        ``do_mask_dev``, read when the launch runs -- with the values of rows ``do_index`` of ``do_table``.

        Returns ``(cf, pa, cf_pa)``: the ``[B, ncol]`` counterfactual table and the ``[B, ctx]`` factual / counterfactual parents
        as the HVAE takes them (``None`` without ``args.parents_x``).  They are static buffers, one set per batch size, valid until
        the next call with as many rows; ``noise(B)`` is the abducted noise of that call.  Only enqueues: inside
        ``torch.cuda.graph`` the tensors passed in are the graph's inputs, their CONTENTS may change between replays.
        ``uniforms``: ``[B, classes]`` f32 per Gumbel-max variable ({variable: tensor}, or the tensor when there is one such
        variable).  Without them, ``rng`` -- the device ``{seed, offset}`` tensor of an engine (``eng.rng`` after ``eng.rng_ptr()``)
        -- fills each such variable's static buffer with one ``cgen_philox_uniform`` launch on the current stream (stream id
        ``989 + k`` for the k-th Gumbel-max mechanism): the state is read when the launch runs and is not advanced, so a replay
        draws at the state's current offset and torch's generators are not touched.  With neither, the uniforms are drawn with
        ``uniform_`` on the device (``generator``), as before.  ``uniforms`` for a variable together with ``rng`` raises."""
        table = self._table(table, "the table")
        index, do_index = self._index(index, "the index"), self._index(do_index, "do_index")
        B = int(index.numel()) if index is not None else int(table.shape[0])
        if B < 1:
            raise ValueError("PgmCounterfactual.run: no rows")
        ent = self._entry(B)
        a = _lib.PgmCfArgs()
        a.obs, a.table_rows, a.index = table.data_ptr(), int(table.shape[0]), None if index is None else index.data_ptr()
        if do_mask_dev is not None:
            if do_vars is not None:
                raise ValueError("PgmCounterfactual.run: give do_vars or do_mask_dev, not both")
            if do_mask_dev.dtype != torch.int32 or do_mask_dev.numel() != 1 or do_mask_dev.device.type != "cuda":
                raise ValueError("PgmCounterfactual.run: do_mask_dev must be a one-element int32 device tensor")
            a.do_mask_dev = do_mask_dev.data_ptr()
        else:
            a.do_mask = self.mask_of(do_vars or ())
        if do_table is not None:
            do_table = self._table(do_table, "do_table")
            a.do_table, a.do_rows, a.do_index = do_table.data_ptr(), int(do_table.shape[0]), None if do_index is None else do_index.data_ptr()
        for t in (table, do_table):
            if t is not None and t.data_ptr() == ent["cf"].data_ptr():
                raise ValueError("PgmCounterfactual.run: the output buffer of an earlier call cannot be an input table (clone it)")
        if self.gumbel:
            if uniforms is not None and not isinstance(uniforms, dict):
                if len(self.gumbel) != 1:
                    raise ValueError("PgmCounterfactual.run: name the Gumbel-max variables of `uniforms` ({variable: tensor})")
                uniforms = {self.vars[self.gumbel[0]]: uniforms}
            if rng is not None:
                if rng.dtype != torch.int64 or rng.numel() != 2 or rng.device.type != "cuda" or not rng.is_contiguous():
                    raise ValueError("PgmCounterfactual.run: rng must be the device {seed, offset} int64 tensor of an engine")
                given = [self.vars[i] for i in self.gumbel if uniforms is not None and uniforms.get(self.vars[i]) is not None]
                if given:
                    raise ValueError(f"PgmCounterfactual.run: give uniforms or rng, not both (uniforms were given for {given})")
            for k, i in enumerate(self.gumbel):
                buf = ent["uniforms"][i]
                u = None if uniforms is None else uniforms.get(self.vars[i])
                if u is None and rng is not None:
                    self.lib.philox_uniform(buf.data_ptr(), buf.numel(), rng.data_ptr(), _lib.STREAM_GUMBEL + k,
                                            torch.cuda.current_stream(self.device).cuda_stream)
                elif u is None:
                    buf.uniform_(generator=generator)
                else:
                    if tuple(u.shape) != tuple(buf.shape):
                        raise ValueError(f"PgmCounterfactual.run: uniforms of {self.vars[i]!r} must be {tuple(buf.shape)}, got {tuple(u.shape)}")
                    buf.copy_(u, non_blocking=True)
                a.uniforms[i] = buf.data_ptr()
        a.cf, a.eps, a.ncol, a.rows, a.exact_gumbel = ent["cf"].data_ptr(), ent["eps"].data_ptr(), self.ncol, B, int(self.exact_gumbel)
        if self.pre:
            a.pa, a.cf_pa, a.npre = ent["pa"].data_ptr(), ent["cf_pa"].data_ptr(), len(self.pre)
            for r, p in zip(a.pre, self.pre):
                r.col, r.width, r.kind, r.hi, r.lo, r.mu, r.sd = p
        self.lib.pgm_counterfactual(self.recs, self.nmech, C.byref(a), torch.cuda.current_stream(self.device).cuda_stream)
        return ent["cf"], ent["pa"], ent["cf_pa"]

    def noise(self, B: int) -> Tensor:
        """``[B, mechanisms]`` abducted noise of the last ``run`` on ``B`` rows (static): the base-distribution value of every
        spline and conditional-affine variable, 0 for roots and Gumbel-max."""
        return self._statics[B]["eps"]


class DevicePGM:
    """What ``DSCM`` and ``CfEvaluator`` ask of a PGM, served by ``PgmCounterfactual``: ``DSCM(args, DevicePGM(pgm), predictor, vae)``
    and ``CfEvaluator(vae, DevicePGM(pgm), predictor, args)`` run their parents through one launch per counterfactual.  Every other
    attribute (``sample``, ``log_prob``, ``state_dict``, ...) is the wrapped PGM's.  After a ``counterfactual`` call
    ``last_parents`` holds the compact ``(pa, cf_pa)`` of ``args.parents_x`` (static buffers; ``None`` without ``args``)."""

    def __init__(self, pgm, args=None, columns=None, ncol=None, exact_gumbel=None, generator=None, device="cuda"):
        self.pgm = pgm
        self.cf = PgmCounterfactual(pgm, args, columns, ncol, exact_gumbel, device)
        self.generator = generator
        self.last_parents = None
        self._tables: Dict[int, Tuple[Tensor, Tensor]] = {}

    def __getattr__(self, name):  # (only reached for what the wrapper itself lacks)
        return getattr(self.__dict__["pgm"], name)

    @property
    def variables(self):
        return self.pgm.variables

    def mechanisms(self):
        return self.pgm.mechanisms()

    def requires_grad_(self, flag: bool = True):
        self.pgm.requires_grad_(flag)
        return self

    def parameters(self):
        return self.pgm.parameters()

    def _fill(self, table: Tensor, values: Dict[str, Tensor], what: str):
        cf = self.cf
        B = table.shape[0]
        for k, v in values.items():
            if k not in cf.width:
                raise ValueError(f"DevicePGM: {what} {k!r} is not a variable of the PGM ({cf.vars})")
            c0, w = cf.columns[k], cf.width[k]
            v = v.detach().reshape(-1, w) if v.dim() != 2 else v.detach()
            if v.shape[1] != w or v.shape[0] not in (1, B):
                raise ValueError(f"DevicePGM: {what} {k!r} of shape {tuple(v.shape)} does not fit [{B}, {w}]")
            table[:, c0:c0 + w].copy_(v, non_blocking=v.is_cuda)

    def _run(self, obs: Dict[str, Tensor], do: Dict[str, Tensor]):
        cf = self.cf
        if set(obs.keys()) != set(self.pgm.variables.keys()):
            raise ValueError(f"DevicePGM: observations {sorted(obs)} are not the PGM's variables {sorted(self.pgm.variables)}")
        B = int(next(iter(obs.values())).shape[0])
        tabs = self._tables.get(B)
        if tabs is None:
            tabs = self._tables[B] = (torch.zeros(B, cf.ncol, device=cf.device), torch.zeros(B, cf.ncol, device=cf.device))
        self._fill(tabs[0], obs, "observation")
        self._fill(tabs[1], do, "intervention")
        out, pa, cf_pa = cf.run(tabs[0], None, tabs[1] if do else None, None, do_vars=list(do), generator=self.generator)
        self.last_parents = (pa, cf_pa)
        return out, B

    @torch.no_grad()
    def counterfactual(self, obs: Dict[str, Tensor], intervention: Dict[str, Tensor], num_particles: int = 1, detach: bool = True) -> Dict[str, Tensor]:
        """``pgm.counterfactual``: {variable: [B, k] device tensor} (fresh tensors, f32).  One particle only."""
        if num_particles != 1:
            raise ValueError(f"DevicePGM.counterfactual: num_particles = {num_particles}; one particle per call is served")
        out, _ = self._run(obs, intervention)
        cf = self.cf
        return {k: out[:, cf.columns[k]:cf.columns[k] + cf.width[k]].clone() for k in obs}

    @torch.no_grad()
    def infer_exogeneous(self, obs: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """{variable + "_base": [B, 1] noise} of every spline and conditional-affine variable (a Gumbel-max variable's posterior
        noise is a draw, not a function of the observation: it is not reported)."""
        _, B = self._run(obs, {})
        eps = self.cf.noise(B)
        return {m.var + "_base": eps[:, i:i + 1].clone() for i, m in enumerate(self.cf.mechs) if m.kind in ("spline", "affine")}
