"""The marginalised cross-entropy kernels of dalm_amd/csrc/ce.hip, element by element, at every kernel form, row alignment and
label edge - and the small kernels of the same file that nothing else calls directly.

Reference (float64, plain torch, on the values the kernel reads - bf16 inputs are up-cast exactly).  Per live row (b, t), with
y = ids[b, t+1] and m = mask[b, t+1]:
    lse = logsumexp(x)      nll = m (lse - x[y])      dlogits = g w (softmax(x) - onehot(y)),   w = m / M  or the row weight
Masked rows (m == 0) and the t = Tg-1 slot are exactly zero.

Bounds.  They are derived from the arithmetic, not measured on the kernels; W = g w is the scale of the row's gradient.
  dlogits, f32  : |got - ref| <= 2e-5 (|ref| + W [element is the label]) for every element; the label element on its own is
                  held to 2e-5 W, every other element to 2e-5 |W softmax|.
                  The exponent fma(x, log2e, -max log2e) is rounded once at a magnitude of up to ~45 (|x - max| < ~30 at
                  logit_gain 3): at most 2^-19 absolute in a base-2 exponent, 1.3e-6 relative in the exponential; the rounding
                  of -max log2e is common to the row and cancels in exp / sum.  An f32 emulation of that formula on the host
                  measured 1.8e-6 up to V = 65544, torch's own f32 softmax 1.2e-6 .. 3.2e-6.  marg_ce_row_kernel and
                  marg_ce_stream_kernel take their gradient this way, as exp(x - max) / sum.
                  marg_ce_row_bf16_kernel (fused, bf16) and marg_ce_bwd_kernel (dalm_marg_ce_bwd, dalm_marg_ce_bwd_weighted)
                  take exp(x - lse) from an f32 lse instead.  That adds the rounding of lse (half a spacing, 2^-24 |lse|,
                  which enters the exponential as it stands) and of -lse log2e (2^-24 |lse| log2e in a base-2 exponent, times
                  ln 2): 2^-23 |lse| relative in all, and nothing of it cancels.  On the rows of logit_gain 3 (|lse| ~ 20) that
                  is 2.4e-6, inside 2e-5; it is only there that these kernels are held to 2e-5.
                  2e-5 leaves room for the hardware exp2 / log / reciprocal (1 ulp each).
  dlogits, bf16 : the same with 2^-8 + 2e-5: one round-to-nearest-even to 8 significant bits (half a spacing is at most 2^-8 of
                  the value, 3.9e-3) on top of the f32 arithmetic.
  dlogits of rows at a large offset (test_rows_shifted_by_a_large_constant): the bounds above for the kernels that take
                  exp(x - max) / sum.  Backward from the saved row_lse is not offset-invariant: an f32 lse of 1e4 is known to
                  4.9e-4 at best, and the C ABI hands the backward kernel nothing else.  There the relative bound is
                  2e-5 + 2^-23 |lse| (f32; 1.2e-3 at 1e4) or 2^-8 + 2e-5 + 2^-23 |lse| (bf16), from the derivation above.
                  The fused bf16 row kernel is held to the same on the bf16 rows shifted by 256.
  row_lse       : |got - ref| <= 1e-5 + 2^-22 max|x_row|  (the absolute tolerance test_hip_parity.py uses, plus one f32 rounding
                  of a value of the row's magnitude); row_nll: the same times m.
  masked rows, the last slot: every element == 0.0, row_lse == row_nll == 0.
  canary        : the logits are a strided view [B, Tg, V] into a 1-D parent buffer (element offset o, row stride st >= V,
                  stride_b >= Tg st).  Every parent element outside the view keeps its sentinel BITS in every mode - the
                  gradient buffer out of place, the logits buffer in place.  The logits parent holds 77.0 there: one element
                  read from a neighbouring row or a gap dominates the row maximum.

Each case prints its largest error / bound per mode (pytest -s).

Kernel forms.  FORMS below restates launch_fwd2: every reachable form is reached by a case, on both sides of every band edge and
one slot below it (test_table_reaches_every_form_and_edge).

One-line changes of ce.hip these tests are meant to catch (what each does to the cases, read off the code):
  (a) launch_fwd2 computes `need` of the unaligned case as V / VEC: the smallest V of every unaligned band (4090, 16378, ... bf16;
      4094, 16382, ... f32) lands in the narrower form, whose registers end one slot early on the rows with a large lead - the
      row's last slot is neither summed nor stored: row_lse out of bound, G_SENTINEL left inside the row.
  (b) marg_ce_row_bf16_kernel does not mask the out-of-row elements of the edge slots: X_SENTINEL from the gap enters the row
      maximum of every unaligned bf16 case above V = 4089: row_lse, row_nll and every gradient element out of bound.
  (c) marg_ce_row_kernel computes slot_y without `lead`: the patch keeps its address and value and only moves to the lane that
      owns the slot before, so the result changes only where that lane's store overtakes the owner's - the label cases on slot
      edges put the two lanes into different waves, but no assertion here can force that order.
"""
import math

import pytest
import torch

import dalm_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
VEC = {F32: 4, BF16: 8}
NAME = {F32: "f32", BF16: "bf16"}
TOL = {F32: 2e-5, BF16: 2.0 ** -8 + 2e-5}
LOSS_RTOL = 1e-4
B, TG = 3, 8
LOGIT_GAIN = 3.0
GSCALE = 0.37
X_SENTINEL = 77.0      # logits parent outside the rows (exact in bf16)
G_SENTINEL = -3.0      # gradient parent before a call (|gradient| <= w <= 1)
ROW_SENTINEL = -7.0    # row_lse / row_nll before a call
TAIL = 16              # parent elements after the last row: the last row's tail slot is read whole


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()  # fail loudly if libdalm_hip.so is absent: no fallback
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# The forms of launch_fwd2 (dalm_amd/csrc/ce.hip).  WHOEVER MOVES A THRESHOLD THERE MOVES THIS TABLE AND `EDGES`.
#   need = V / VEC                      (ALIGNED: base pointer, V, stride_b, stride_t all on 16 bytes)
#        = (V + 2 (VEC - 1)) / VEC      (otherwise: the slot count with the worst-case lead)
#   (largest `need`, kernel, BS, SLOTS) in the order the launcher tests them; None = everything above
# ---------------------------------------------------------------------------------------------------------------------
FORMS = {
    F32: ((256 * 4, "row", 256, 4), (256 * 16, "row", 256, 16), (512 * 16, "row", 512, 16), (1024 * 16, "row", 1024, 16),
          (None, "stream", 1024, 0)),
    BF16: ((256 * 2, "row", 256, 2), (512 * 4, "row_bf16", 512, 4), (512 * 8, "row_bf16", 512, 8), (1024 * 8, "row_bf16", 1024, 8),
           (None, "stream", 1024, 0)),
}
BF16_FWD_ONLY_STREAMS_FROM = 8192   # forward-only bf16 rows: the streaming kernel from this V, whatever the alignment


def need_slots(dtype, aligned, V):
    v = VEC[dtype]
    return V // v if aligned else (V + 2 * (v - 1)) // v


def form_of(dtype, grad, aligned, V):
    if not grad and dtype is BF16 and V >= BF16_FWD_ONLY_STREAMS_FROM:
        return ("stream", 1024, 0)
    need = need_slots(dtype, aligned, V)
    for top, kernel, bs, slots in FORMS[dtype]:
        if top is None or need <= top:
            return (kernel, bs, slots)
    raise AssertionError


# "largest V of a band | smallest V of the next"
EDGES = {
    (BF16, True): ((4096, 4104), (16384, 16392), (32768, 32776), (65536, 65544)),
    (BF16, False): ((4089, 4090), (16377, 16378), (32761, 32762), (65529, 65530)),
    (F32, True): ((4096, 4100), (16384, 16388), (32768, 32772), (65536, 65540)),
    (F32, False): ((4093, 4094), (16381, 16382), (32765, 32766), (65533, 65534)),
}
# forward-only bf16: the bands up to 8191, the streaming kernel from 8192
FWD_ONLY_EDGES = {(BF16, True): ((8184, 8192),), (BF16, False): ((8191, 8193),)}
TINY = (5, 200)        # smaller than one slot; smaller than a block
LAYOUTS = {True: ("aligned",), False: ("odd", "maxlead")}


def _case_list():
    cases = []
    for dtype in (F32, BF16):
        for aligned in (True, False):
            vs = []
            for lo, hi in EDGES[(dtype, aligned)] + FWD_ONLY_EDGES.get((dtype, aligned), ()):
                vs += [lo - VEC[dtype], lo, hi]
            if dtype is BF16 and not aligned:
                vs.append(8192)     # the forward-only threshold itself on unaligned rows
            vs += [v for v in TINY if not aligned or v % VEC[dtype] == 0]
            for kind in LAYOUTS[aligned]:
                for V in sorted(set(vs)):
                    cases.append((dtype, kind, V, None))
    # the gradient buffer on another 16-byte phase than the logits (the kernel takes `lead` from the logits row only)
    cases.append((F32, "maxlead", 4094, 1))
    cases.append((BF16, "maxlead", 4090, 1))
    return cases


CASES = _case_list()


def _case_id(c):
    dtype, kind, V, og = c
    return f"{NAME[dtype]}-{kind}-{V}" + ("" if og is None else f"-gphase{og}")


class Layout:
    """Logits [B, TG, V] as a strided view into a 1-D parent: element offset o, row stride st, sample stride sb."""

    def __init__(self, dtype, kind, V, og=None):
        v = VEC[dtype]
        self.dtype, self.kind, self.V, self.vec = dtype, kind, V, v
        up = -(-V // v) * v
        if kind == "aligned":
            assert V % v == 0
            self.o, self.st = 0, V + v
            self.sb = TG * self.st + v
        elif kind == "odd":          # the lead of consecutive rows cycles through all VEC values
            self.o, self.st = 1, V + 1 + (V % 2)
            self.sb = TG * self.st + 5
            assert self.st % 2 == 1
        elif kind == "maxlead":      # every row has the largest lead
            self.o, self.st = v - 1, up + v
            self.sb = TG * self.st + v
        else:
            raise AssertionError(kind)
        self.og = self.o if og is None else og
        self.aligned = kind == "aligned"
        assert self.st >= V and self.sb >= TG * self.st
        bt = torch.arange(B).unsqueeze(1) * self.sb + torch.arange(TG).unsqueeze(0) * self.st
        self.row_off = bt                                    # without o / og
        self.lead = (self.o + bt) % v                        # parents are 16-byte aligned (asserted at allocation)
        self.nslots = (self.lead + V + v - 1) // v
        self.span = int(bt.max()) + V + TAIL

    def parent(self, dev, fill, off):
        p = torch.full((off + self.span,), fill, dtype=self.dtype, device=dev)
        assert p.data_ptr() % 16 == 0
        return p

    def view(self, parent, off):
        return parent.as_strided((B, TG, self.V), (self.sb, self.st, 1), off)

    def inside(self, dev, off):
        idx = (off + self.row_off.to(dev)).unsqueeze(2) + torch.arange(self.V, device=dev)
        m = torch.zeros(off + self.span, dtype=torch.bool, device=dev)
        m[idx.reshape(-1)] = True
        return m


def bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def canary_intact(parent, inside, sentinel):
    want = bits(torch.tensor([sentinel], dtype=parent.dtype))[0].item()
    return bool(((bits(parent) == want) | inside).all())


def default_mask():
    """Sample 0 full, sample 1 left-padded by 3, sample 2 right-padded by 2: live rows, masked rows and the last slot."""
    mask = torch.ones(B, TG, dtype=torch.int64)
    mask[1, :3] = 0
    mask[2, TG - 2:] = 0
    return mask


def place_labels(ids, live, lay, bs):
    """Random labels, but the first live rows carry the edge positions: 0, V-1, the last element of the row's head slot, the first
    of its tail slot, and both sides of BS VEC, where the label passes from one register slot of a lane to the next (counted in
    the row's 16-byte window, i.e. minus its lead, and as a plain index)."""
    V, v = lay.V, lay.vec
    k = 0
    for b in range(B):
        for t in range(TG - 1):
            if not live[b, t]:
                continue
            ld, ns = int(lay.lead[b, t]), int(lay.nslots[b, t])
            cands = [0, V - 1, v - 1 - ld, (ns - 1) * v - ld, bs * v - 1 - ld, bs * v - ld, bs * v - 1, bs * v]
            if k < len(cands) and 0 <= cands[k] < V:
                ids[b, t + 1] = cands[k]
            k += 1
    return ids


def reference(x, ids, mask):
    """float64 reference on the host.  x [B,TG,V] (any float dtype, read exactly).  Returns a dict of float64 / bool tensors."""
    x = x.double()
    m = torch.zeros(B, TG, dtype=torch.float64)
    m[:, :-1] = mask[:, 1:].double()
    y = torch.zeros(B, TG, dtype=torch.int64)
    y[:, :-1] = ids[:, 1:]
    live = m != 0
    V = x.shape[2]
    y_ok = (y >= 0) & (y < V) & live
    lse = torch.where(live, torch.logsumexp(x, 2), torch.zeros(()).double())
    xy = torch.gather(x, 2, y.clamp(0, V - 1).unsqueeze(2)).squeeze(2)
    nll = torch.where(live, m * (lse - xy), torch.zeros(()).double())
    nll = torch.where(live & ~y_ok, torch.full((), float("nan")).double(), nll)
    soft = torch.softmax(x, 2) * live.unsqueeze(2)
    onehot = torch.zeros_like(soft)
    onehot.scatter_(2, y.clamp(0, V - 1).unsqueeze(2), y_ok.unsqueeze(2).double())
    xmax = x.masked_fill(torch.isinf(x), 0.0).abs().amax(2)
    return {"m": m, "y": y, "live": live, "y_ok": y_ok, "lse": lse, "nll": nll, "soft": soft, "onehot": onehot, "xmax": xmax,
            "M": m.sum()}


class Checker:
    """Holds the reference on the device and applies the bounds of the module docstring."""

    def __init__(self, ref, dtype, dev, name):
        self.r = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in ref.items()}
        self.tol, self.name, self.figures = TOL[dtype], name, {}

    def rows(self, mode, lse, nll):
        r = self.r
        lse, nll = lse.reshape(B, TG).double(), nll.reshape(B, TG).double()
        dead = ~r["live"]
        assert bool((lse[dead] == 0).all()) and bool((nll[dead] == 0).all()), f"{self.name} {mode}: masked row_lse/row_nll not 0"
        bound = 1e-5 + 2.0 ** -22 * r["xmax"]
        e_lse = (lse - r["lse"]).abs()[r["live"]]
        assert bool(torch.isfinite(lse).all())
        ratio = float((e_lse / bound[r["live"]]).max())
        self.figures[f"{mode}.lse"] = ratio
        assert ratio <= 1.0, f"{self.name} {mode}: row_lse error / bound = {ratio:.3g}"
        ok = r["live"] & r["y_ok"]
        nan_rows = r["live"] & ~r["y_ok"]
        assert bool(torch.isnan(nll[nan_rows]).all()), f"{self.name} {mode}: row_nll of an out-of-range label must be NaN"
        assert bool(torch.isfinite(nll[ok]).all())
        ratio = float(((nll - r["nll"]).abs()[ok] / (bound * r["m"])[ok]).max())
        self.figures[f"{mode}.nll"] = ratio
        assert ratio <= 1.0, f"{self.name} {mode}: row_nll error / bound = {ratio:.3g}"

    def grad(self, mode, got, W, lse_term=False):
        """got [B,TG,V] (the row elements), W [B,TG] float64 = g w on live rows (anything on dead rows).  lse_term adds
        2^-23 |lse| of the row to the relative bound (module docstring: gradients taken as exp(x - lse) from an f32 lse)."""
        r = self.r
        tol = self.tol + (2.0 ** -23 * r["lse"].abs()).unsqueeze(2) if lse_term else self.tol
        got = got.double()
        assert bool(torch.isfinite(got).all()), f"{self.name} {mode}: non-finite gradient"
        W = (W.to(got.device) * r["live"]).unsqueeze(2)
        dead = ~r["live"]
        assert bool((got[dead] == 0).all()), f"{self.name} {mode}: masked rows / the last slot are not exactly 0"
        ref = W * (r["soft"] - r["onehot"])
        err = (got - ref).abs()
        # every element
        bound = tol * (ref.abs() + W * r["onehot"])
        bad = err > bound
        if bool(bad.any()):
            i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{self.name} {mode}: {int(bad.sum())} elements out of bound, first (b,t,v)={i} "
                                 f"got {got[tuple(i)].item():.9g} ref {ref[tuple(i)].item():.9g} bound {bound[tuple(i)].item():.3g}")
        # the label element on its own against tol W, every other element against tol |W softmax|
        lab = r["onehot"] != 0
        e_lab = (err / (tol * W).clamp_min(1e-300)).expand_as(err)[lab]
        if e_lab.numel():
            self.figures[f"{mode}.label"] = float(e_lab.max())
            assert float(e_lab.max()) <= 1.0, f"{self.name} {mode}: label element error / (tol W) = {float(e_lab.max()):.3g}"
        other = tol * W * r["soft"]
        bad = (err > other) & ~lab
        assert not bool(bad.any()), f"{self.name} {mode}: a non-label element differs from W softmax, first {torch.nonzero(bad)[0].tolist()}"
        nz = (other > 0) & ~lab
        self.figures[f"{mode}.rest"] = float((err[nz] / other[nz]).max()) if bool(nz.any()) else 0.0


def make_inputs(dtype, lay, mask, seed, bs):
    g = torch.Generator().manual_seed(seed)
    x = (LOGIT_GAIN * torch.randn(B, TG, lay.V, generator=g)).to(dtype)
    ids = torch.randint(0, lay.V, (B, TG), generator=g)
    live = torch.zeros(B, TG, dtype=torch.bool)
    live[:, :-1] = mask[:, 1:] != 0
    ids = place_labels(ids, live, lay, bs)
    rw = torch.rand(B * TG, generator=g) + 0.1
    return x, ids, rw


def run_modes(dev, lay, x, ids, mask, rw, name, ref=None, lse_term=()):
    """Run the kernels on one set of inputs and check every mode: the fused forward out of place, a second identical call, in
    place, forward-only, dalm_marg_ce_bwd and dalm_marg_ce_bwd_weighted.  `lse_term` names the modes whose gradient bound
    carries the 2^-23 |lse| term.  Returns (Checker, fused gradient rows)."""
    modes = ("fused", "again", "inplace", "fwd_only", "bwd", "bwd_weighted")
    from dalm_amd import hip
    from dalm_amd.ops import default_ops

    ops = default_ops()
    dtype, V = lay.dtype, lay.V
    code = hip.dtype_code(x)
    ref = ref or reference(x, ids, mask)
    ck = Checker(ref, dtype, dev, name)
    xp = lay.parent(dev, X_SENTINEL, lay.o)
    xv = lay.view(xp, lay.o)
    xv.copy_(x.to(dev))
    x_inside, g_inside = lay.inside(dev, lay.o), lay.inside(dev, lay.og)
    ids_d, mask_d, rw_d = ids.to(dev), mask.to(dev), rw.to(dev)
    gs = torch.tensor([GSCALE], device=dev)
    g32 = float(torch.tensor(GSCALE, dtype=F32).double())
    stats, _, _ = ops.ce_prep(mask_d, None)
    assert float(stats[0]) == float(ref["M"])
    W = ref["m"] / ref["M"]
    common = (B, TG, V, lay.sb, lay.st, hip.ptr(ids_d), hip.ptr(mask_d), hip.ptr(stats))

    def rows_buf():
        return torch.full((B * TG,), ROW_SENTINEL, device=dev), torch.full((B * TG,), ROW_SENTINEL, device=dev)

    def fused():
        gp = lay.parent(dev, G_SENTINEL, lay.og)
        lse, nll = rows_buf()
        hip.call("dalm_marg_ce_fwd", hip.ptr(xv), code, *common, hip.ptr(lse), hip.ptr(nll), hip.ptr(lay.view(gp, lay.og)),
                 hip.stream())
        return gp, lse, nll

    gp, lse, nll = fused()
    dl = lay.view(gp, lay.og).contiguous()
    if "fused" in modes:
        ck.rows("fused", lse, nll)
        ck.grad("fused", dl, W, "fused" in lse_term)
        assert canary_intact(gp, g_inside, G_SENTINEL), f"{name} fused: a gradient store left the rows"
        assert torch.equal(bits(xp), bits(_filled(lay, dev, x))), f"{name} fused: the logits were written out of place"
    if "again" in modes:       # a second identical call gives identical bits, canary included
        gp2, lse2, nll2 = fused()
        assert torch.equal(bits(gp2), bits(gp)) and torch.equal(bits(lse2), bits(lse)) and torch.equal(bits(nll2), bits(nll)), \
            f"{name}: two identical calls differ"
    if "inplace" in modes:     # dlogits aliases the logits (a copy): the same bits as out of place, gaps untouched
        xp2 = xp.clone()
        xv2 = lay.view(xp2, lay.o)
        lse3, nll3 = rows_buf()
        hip.call("dalm_marg_ce_fwd", hip.ptr(xv2), code, *common, hip.ptr(lse3), hip.ptr(nll3), hip.ptr(xv2), hip.stream())
        assert torch.equal(bits(xv2.contiguous()), bits(dl)), f"{name} inplace: differs from the out-of-place gradient"
        assert torch.equal(bits(lse3), bits(lse)) and torch.equal(bits(nll3), bits(nll)), f"{name} inplace: row_lse / row_nll differ"
        assert canary_intact(xp2, x_inside, X_SENTINEL), f"{name} inplace: a gradient store left the rows"
    if "fwd_only" in modes:
        lse4, nll4, none = ops.ce_fwd(xv, ids_d, mask_d, stats, False)
        assert none is None
        ck.rows("fwd_only", lse4, nll4)
    for mode in ("bwd", "bwd_weighted"):
        if mode not in modes:
            continue
        gp5 = lay.parent(dev, G_SENTINEL, lay.og)
        out = hip.ptr(lay.view(gp5, lay.og))
        if mode == "bwd":
            hip.call("dalm_marg_ce_bwd", hip.ptr(xv), code, *common, hip.ptr(lse), hip.ptr(gs), out, hip.stream())
            Wm = g32 * W
        else:
            hip.call("dalm_marg_ce_bwd_weighted", hip.ptr(xv), code, *common, hip.ptr(lse), hip.ptr(gs), hip.ptr(rw_d), out,
                     hip.stream())
            Wm = g32 * rw.double().reshape(B, TG)
        ck.grad(mode, lay.view(gp5, lay.og).contiguous(), Wm, mode in lse_term)
        assert canary_intact(gp5, g_inside, G_SENTINEL), f"{name} {mode}: a gradient store left the rows"
    print(f"\n[ce_forms] {name}: error/bound " + " ".join(f"{k}={v:.3g}" for k, v in ck.figures.items()))
    return ck, dl


def _filled(lay, dev, x):
    p = lay.parent(dev, X_SENTINEL, lay.o)
    lay.view(p, lay.o).copy_(x.to(dev))
    return p


def _seed(dtype, kind, V):
    return 1000003 * V + 17 * sorted(LAYOUTS[True] + LAYOUTS[False]).index(kind) + (dtype is BF16)


# ---------------------------------------------------------------------------------------------------------------------
# Every forward form, both sides of every band edge, every mode, labels on the slot edges
# ---------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_form_and_edge():
    """The case table against FORMS: every form the launcher can reach is reached, and each edge separates two forms with the
    value one slot below still inside the lower band."""
    reached = set()
    for dtype, kind, V, _ in CASES:
        for grad in (True, False):
            kernel, bs, slots = form_of(dtype, grad, kind == "aligned", V)
            reached.add((dtype, grad, kernel, bs, slots, kind == "aligned" or kernel == "stream"))
            if kernel == "stream":
                reached.add((dtype, grad, kernel, bs, slots, False))
    want = set()
    for dtype in (F32, BF16):
        for grad in (True, False):
            for _, kernel, bs, slots in FORMS[dtype]:
                if dtype is BF16 and not grad and kernel == "row_bf16" and slots == 8:
                    continue    # need <= 512*4 holds up to V = 16384, and forward-only bf16 streams from 8192: never launched
                for aligned in (True, False):
                    want.add((dtype, grad, kernel, bs, slots, aligned))
    assert reached == want, (sorted(map(str, want - reached)), sorted(map(str, reached - want)))
    for table, grads in ((EDGES, (True,)), (FWD_ONLY_EDGES, (False,))):
        for (dtype, aligned), pairs in table.items():
            for lo, hi in pairs:
                for grad in grads:
                    assert form_of(dtype, grad, aligned, lo) != form_of(dtype, grad, aligned, hi), (NAME[dtype], aligned, lo, hi)
                    assert form_of(dtype, grad, aligned, lo - VEC[dtype]) == form_of(dtype, grad, aligned, lo)
                    if not aligned and table is EDGES:     # largest V of the band: with the largest lead the row fills the band's last slot
                        assert (lo + VEC[dtype] - 1) == need_slots(dtype, False, lo) * VEC[dtype]
    # f32 forward-only takes the same bands as the gradient form
    for (dtype, aligned), pairs in EDGES.items():
        if dtype is F32:
            for lo, hi in pairs:
                assert form_of(dtype, False, aligned, lo) != form_of(dtype, False, aligned, hi)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_ce_forms(dev, case):
    dtype, kind, V, og = case
    lay = Layout(dtype, kind, V, og)
    mask = default_mask()
    live = torch.zeros(B, TG, dtype=torch.bool)
    live[:, :-1] = mask[:, 1:] != 0
    v = VEC[dtype]
    if kind == "odd":       # every lead occurs on a live row; a full and a partial tail slot both occur
        assert sorted(set(lay.lead[live].tolist())) == list(range(v))
        tails = ((lay.lead + V) % v)[live]
        assert bool((tails == 0).any()) and bool((tails != 0).any())
    elif kind == "maxlead":
        assert bool((lay.lead == v - 1).all()) and (lay.o * lay.dtype.itemsize) % 16 != 0 and lay.st % v == 0 and lay.sb % v == 0
    else:
        assert bool((lay.lead == 0).all()) and lay.st % v == 0 and lay.sb % v == 0 and V % v == 0
    if og is not None:
        assert (og - lay.o) % v != 0
    bs = form_of(dtype, True, lay.aligned, V)[1]
    x, ids, rw = make_inputs(dtype, lay, mask, _seed(dtype, kind, V), bs)
    run_modes(dev, lay, x, ids, mask, rw, _case_id(case))


# ---------------------------------------------------------------------------------------------------------------------
# Values at the edges - one register-resident and one streaming V per dtype (unaligned rows, every lead)
# ---------------------------------------------------------------------------------------------------------------------
EDGE_V = [(F32, 4999), (F32, 65541), (BF16, 5001), (BF16, 65545)]
_edge = pytest.mark.parametrize("dtype,V", EDGE_V, ids=[f"{NAME[d]}-{v}" for d, v in EDGE_V])


def _edge_setup(dtype, V, mask=None):
    lay = Layout(dtype, "odd", V)
    mask = default_mask() if mask is None else mask
    bs = form_of(dtype, True, False, V)[1]
    x, ids, rw = make_inputs(dtype, lay, mask, _seed(dtype, "odd", V) + 1, bs)
    return lay, mask, x, ids, rw


def _put_neg_inf(lay, x, ids):
    v, V = lay.vec, lay.V
    bs = form_of(lay.dtype, True, False, V)[1]      # thread 9 owns the slots 9, 9 + BS, 9 + 2 BS, ... of the form that runs
    g = torch.Generator().manual_seed(V)
    for b in range(B):
        for t in range(TG):
            ld = int(lay.lead[b, t])
            row = x[b, t]
            y = int(ids[b, min(t + 1, TG - 1)])
            keep = row[y].clone()
            row[torch.rand(V, generator=g) < 1 / 64] = -math.inf
            row[: max(0, 3 * v - ld)] = -math.inf                        # slots 0..2
            row[max(0, 5 * v - ld): 6 * v - ld] = -math.inf              # thread 5: its first slot
            for s in range(9, int(lay.nslots[b, t]), bs):                # thread 9: everything it sees
                row[max(0, s * v - ld): s * v - ld + v] = -math.inf
            row[y] = keep


def test_edge_values_reach_both_kinds_of_kernel():
    for dtype, V in EDGE_V:
        assert (form_of(dtype, True, False, V)[0] == "stream") == (V > 65000)


@_edge
def test_neg_inf_entries(dev, dtype, V):
    """-inf away from the label: the whole first slot of one thread (in the streaming kernel its running maximum is still
    -inf after it), every slot that thread 9 of the gradient form's block owns, the first three slots of the row, and one
    entry in 64 at random."""
    lay, mask, x, ids, rw = _edge_setup(dtype, V)
    _put_neg_inf(lay, x, ids)
    ck, dl = run_modes(dev, lay, x, ids, mask, rw, f"neginf-{NAME[dtype]}-{V}")
    assert bool(torch.isfinite(dl).all())


SHIFTS = [(F32, 4999, 1e4), (F32, 65541, 1e4), (BF16, 5001, 3e4), (BF16, 65545, 3e4), (BF16, 5001, 256.0), (BF16, 65545, 256.0)]


@pytest.mark.parametrize("dtype,V,shift", SHIFTS, ids=[f"{NAME[d]}-{v}-{s:g}" for d, v, s in SHIFTS])
def test_rows_shifted_by_a_large_constant(dev, dtype, V, shift):
    """x + 1e4 (f32), x + 3e4 and x + 256 (bf16), as the dtype holds it: the gradient is that of the unshifted row (the same
    values minus the constant, exact in the dtype); row_lse within its bound, whose second term exists for this case.

    bf16 at 3e4 has a spacing of 128: every logit becomes 29952, the rows are constant and softmax is 1 / V - one value per
    row.  At 256 the spacing is 1 below and 2 above, and the rows keep their structure.

    The fused forward with gradient holds the bound of every other test at 1e4 and 3e4.  dalm_marg_ce_bwd and
    dalm_marg_ce_bwd_weighted see the row only through the saved f32 row_lse, so their bound carries the 2^-23 |lse| term
    of the module docstring (1.2e-3 at 1e4, 3.6e-3 at 3e4): backward from row_lse is not offset-invariant.  The bf16 rows at
    256 carry the term (3.2e-5) in the fused mode too: marg_ce_row_bf16_kernel recomputes exp(x - lse) for its gradient."""
    lay, mask, x, ids, rw = _edge_setup(dtype, V)
    xs = (x.float() + shift).to(dtype)
    assert float(xs.double().max() - xs.double().min()) < 60     # the documented logit range: nothing underflows in f32
    c = float(xs.double().min()) if shift == 3e4 else shift      # bf16 at 3e4: subtract a value of the grid
    base = (xs.double() - c).to(dtype)
    assert torch.equal(base.double() + c, xs.double())           # the unshifted row is exact in the dtype
    assert (int(base.unique().numel()) == 1) == (shift == 3e4)   # only the rows at 3e4 are constant
    ref = reference(base, ids, mask)                              # the UNSHIFTED row's gradient ...
    ref_s = reference(xs, ids, mask)
    torch.testing.assert_close(ref_s["soft"], ref["soft"], rtol=1e-9, atol=0)
    ref["lse"], ref["nll"], ref["xmax"] = ref_s["lse"], ref_s["nll"], ref_s["xmax"]     # ... the shifted row's lse
    lse_term = ("bwd", "bwd_weighted") + (("fused",) if shift == 256.0 else ())
    run_modes(dev, lay, xs, ids, mask, rw, f"shift-{NAME[dtype]}-{V}-{shift:g}", ref=ref, lse_term=lse_term)


@_edge
def test_integer_mask_weights_above_one(dev, dtype, V):
    mask = default_mask()
    mask[0, 1:5] = torch.tensor([2, 3, 1, 5])
    mask[2, 2] = 4
    lay, mask, x, ids, rw = _edge_setup(dtype, V, mask)
    ck, _ = run_modes(dev, lay, x, ids, mask, rw, f"weights-{NAME[dtype]}-{V}")
    assert float(ck.r["M"]) == float(mask[:, 1:].sum()) and float(ck.r["m"].max()) == 5.0


@_edge
@pytest.mark.parametrize("bad", ["V", "-1"])
def test_label_out_of_range_on_one_row(dev, dtype, V, bad):
    """That row's row_nll is NaN and its gradient w softmax with no patch; every other row and the canary are as always."""
    lay, mask, x, ids, rw = _edge_setup(dtype, V)
    ids[0, 3] = V if bad == "V" else -1        # row (0, 2): live
    ck, _ = run_modes(dev, lay, x, ids, mask, rw, f"badlabel{bad}-{NAME[dtype]}-{V}")
    assert int((ck.r["live"] & ~ck.r["y_ok"]).sum()) == 1


@_edge
def test_every_target_masked(dev, dtype, V):
    """M == 0: 0 * (1/M) is NaN in every row t < Tg-1 and exactly 0 at t = Tg-1 (closed_backward of oracle/dalm_oracle.py gives
    the same pattern); row_lse = row_nll = 0; nothing outside the rows is written."""
    from dalm_amd import hip
    from dalm_amd.ops import default_ops

    mask = torch.zeros(B, TG, dtype=torch.int64)
    mask[:, 0] = 1      # only column 0 - never a target
    lay, mask, x, ids, rw = _edge_setup(dtype, V, mask)
    q = torch.zeros(B, 4, dtype=torch.float64)
    oracle = O.closed_backward(q, q, x[:, :, :64].double(), ids % 64, mask, torch.ones(B, dtype=torch.int64), 1.0)["dlogits"]
    assert bool(torch.isnan(oracle[:, :-1]).all()) and bool((oracle[:, -1] == 0).all())
    ops = default_ops()
    xp = _filled(lay, dev, x)
    xv = lay.view(xp, lay.o)
    ids_d, mask_d = ids.to(dev), mask.to(dev)
    stats, _, _ = ops.ce_prep(mask_d, None)
    assert float(stats[0]) == 0.0
    inside = lay.inside(dev, lay.o)
    common = (hip.dtype_code(x), B, TG, V, lay.sb, lay.st, hip.ptr(ids_d), hip.ptr(mask_d), hip.ptr(stats))
    lse = torch.full((B * TG,), ROW_SENTINEL, device=dev)
    nll = torch.full((B * TG,), ROW_SENTINEL, device=dev)
    gs = torch.tensor([GSCALE], device=dev)
    for mode in ("fused", "bwd"):
        gp = lay.parent(dev, G_SENTINEL, lay.o)
        if mode == "fused":
            hip.call("dalm_marg_ce_fwd", hip.ptr(xv), *common, hip.ptr(lse), hip.ptr(nll), hip.ptr(lay.view(gp, lay.o)), hip.stream())
            assert bool((lse == 0).all()) and bool((nll == 0).all())
        else:
            hip.call("dalm_marg_ce_bwd", hip.ptr(xv), *common, hip.ptr(lse), hip.ptr(gs), hip.ptr(lay.view(gp, lay.o)), hip.stream())
        dl = lay.view(gp, lay.o)
        assert bool(torch.isnan(dl[:, :-1]).all()), mode
        assert bool((dl[:, -1] == 0).all()), mode
        assert canary_intact(gp, inside, G_SENTINEL), mode


# ---------------------------------------------------------------------------------------------------------------------
# The small kernels of ce.hip that nothing calls directly
# ---------------------------------------------------------------------------------------------------------------------
def _qlens(Tg):
    return [-Tg - 3, -1, 0, 1, 2, Tg - 1, Tg, Tg + 5]


@pytest.mark.parametrize("Tg", [70, 2, 130])
def test_prep_vs_python_slices(dev, Tg):
    """Nb / Mb / stats against python slicing of the Tg-1 shifted rows, lp[qlen-1:]; B = 300 takes the total round its loop."""
    from dalm_amd import hip

    Bn = 300
    g = torch.Generator().manual_seed(Tg)
    mask = torch.randint(0, 3, (Bn, Tg), generator=g)
    ql = _qlens(Tg)
    qlen = torch.tensor([ql[i % len(ql)] for i in range(Bn)])
    rows = [mask[b, 1:].tolist() for b in range(Bn)]
    want_Mb = torch.tensor([float(sum(r)) for r in rows])
    want_Nb = torch.tensor([float(sum(r[int(q) - 1:])) for r, q in zip(rows, qlen)])
    mask_d, qlen_d = mask.to(dev), qlen.to(dev)
    for q_d, want in ((qlen_d, want_Nb), (None, torch.zeros(Bn))):      # qlen = NULL: no answer rows
        stats = torch.full((2,), ROW_SENTINEL, device=dev)
        Nb, Mb = torch.full((Bn,), ROW_SENTINEL, device=dev), torch.full((Bn,), ROW_SENTINEL, device=dev)
        hip.call("dalm_marg_ce_prep", hip.ptr(mask_d), hip.ptr(q_d), Bn, Tg, hip.ptr(stats), hip.ptr(Nb), hip.ptr(Mb), hip.stream())
        assert torch.equal(Mb.cpu(), want_Mb) and torch.equal(Nb.cpu(), want)
        assert stats.tolist() == [float(want_Mb.double().sum()), float(Bn)]


@pytest.mark.parametrize("with_doc", [True, False])
def test_finalize_vs_fp64_sum(dev, with_doc):
    from dalm_amd import hip

    R, Bn = 2500, 1100
    g = torch.Generator().manual_seed(R + with_doc)
    row_nll = torch.rand(R, generator=g) * 9
    Nb = torch.randint(0, 40, (Bn,), generator=g).float()
    doc = -torch.rand(Bn, generator=g) * 4
    stats = torch.tensor([1234.0, float(Bn)])
    want = row_nll.double().sum()
    if with_doc:
        want = want - (Nb.double() * doc.double()).sum()
    want = float(want / 1234.0)
    out = torch.full((1,), ROW_SENTINEL, device=dev)
    d = [t.to(dev) for t in (row_nll, Nb, doc, stats)]
    hip.call("dalm_marg_ce_finalize", hip.ptr(d[0]), R, hip.ptr(d[1]), hip.ptr(d[2]) if with_doc else None, Bn, hip.ptr(d[3]),
             hip.ptr(out), hip.stream())
    assert abs(float(out) - want) <= LOSS_RTOL * abs(want), (float(out), want)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", ["lt_vec", "ragged", "grid_cap"])
def test_scale_inplace(dev, dtype, n):
    """gscale == 1 leaves every bit; otherwise x g rounded once to the dtype (bf16: through the f32 product, so the distance to
    the exact product is at most half a bf16 spacing plus half an f32 one)."""
    from dalm_amd.ops import default_ops

    v = VEC[dtype]
    n = {"lt_vec": v - 1, "ragged": 1000 * v + v - 1, "grid_cap": (4096 * 256 + 5 * 256 + 7) * v + v - 2}[n]
    g = torch.Generator().manual_seed(n)
    x = (4 * torch.randn(n, generator=g)).to(dtype)
    ops = default_ops()
    xd = x.to(dev)
    ops.scale_inplace(xd, torch.tensor([1.0], device=dev))
    assert torch.equal(bits(xd.cpu()), bits(x))
    gsc = torch.tensor([GSCALE])
    ops.scale_inplace(xd, gsc.to(dev))
    got = xd.cpu()
    exact = x.double() * gsc.double()
    if dtype is F32:
        assert torch.equal(bits(got), bits(exact.float()))      # float64 -> float32 of an exact product: rounded once
    else:
        spacing = torch.ldexp(torch.ones(()).double(), torch.frexp(exact)[1] - 8)     # bf16: 8 significant bits
        assert bool(((got.double() - exact).abs() <= 0.5 * spacing * (1 + 2.0 ** -15)).all())
        assert torch.equal(bits(got), bits((x.float() * gsc).to(BF16)))


def test_gather_nll(dev):
    from dalm_amd.ops import default_ops

    R, V = 700, 37
    g = torch.Generator().manual_seed(R)
    lp = -torch.rand(R, V, generator=g) * 8
    labels = torch.randint(0, V, (R,), generator=g)
    bad = {3: -1, 255: V, 256: V + 5, 699: -V}
    for r, y in bad.items():
        labels[r] = y
    got = default_ops().gather_nll(lp.to(dev), labels.to(dev)).cpu()
    ok = torch.ones(R, dtype=torch.bool)
    ok[list(bad)] = False
    assert bool(torch.isnan(got[~ok]).all())
    assert torch.equal(got[ok], -lp[torch.arange(R), labels.clamp(0, V - 1)][ok])


def test_marginalize_rows_both_entry_points(dev):
    """T V beyond the reach of the 8192 x 256 grid: the grid-stride loop runs twice."""
    from dalm_amd.ops import default_ops

    T, V = 33, 70001
    assert T * V > 8192 * 256
    ops = default_ops()
    g = torch.Generator().manual_seed(T)
    lp = -torch.rand(T, V, generator=g) * 5
    doc = torch.tensor([-1.25])
    lp_d, doc_d = lp.to(dev), doc.to(dev)
    for ql in _qlens(T + 1):
        want = O.ref_marginalize_log_probs(lp.double(), doc.double(), ql)
        assert want.shape == (T, V)
        for q in (ql, torch.tensor([ql, 99], device=dev)[0]):
            got = ops.marginalize_rows(lp_d, doc_d, q)
            torch.testing.assert_close(got.cpu().double(), want, rtol=0, atol=1e-6)
