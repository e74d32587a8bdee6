"""The LoRA group node's forward on ONE buffer (models/lora_ops.py, models/frozen_linear.py): q | k | v as one GEMM into
[R, sum N] whose column slices are the outputs, the rank updates in place on the slices (`dalm_lora2_rankupd_ld`).  The backward
is the accumulating route it was.

Three layouts (those of test_lora2_gpu.py's group test: Llama q / v adapters, grouped-query with a narrower k / v, BERT with three
adapters and biases) at K = 256, R = 96, the one-GEMM route against the three-GEMM route (`frozen_linear._CAT` cleared) and
against float64:
* forward inside the bounds of test_lora2_gpu.py (route against route: out < 8e-3; against float64: 4e-3), and the one-GEMM
  route's largest error against float64 no larger than the three-GEMM route's plus one bf16 ulp of the largest element;
* dx, the lora_A / lora_B gradients and the dropout mask bytes BIT-identical between the routes: the backward and the branch run
  the same calls on the same operands;
* through the attention kernels (views of the slices as heads) and with one output's gradient `None`: dx within 1.2e-2 of the
  three-GEMM route's;
* the state_dict is unchanged by the concatenation, `uncat_weights` separates the storages again, and three Adam steps with
  dropout replayed from a `torch.cuda.graph` match the eager steps without a parameter being re-pointed inside the capture."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K, R, HD = 256, 96, 64
LAYOUTS = [
    pytest.param(("q_proj", "k_proj", "v_proj"), ["q_proj", "v_proj"], 256, 256, False, id="llama"),
    pytest.param(("q_proj", "k_proj", "v_proj"), ["q_proj", "v_proj"], 256, 128, False, id="grouped-query"),
    pytest.param(("query", "key", "value"), ["key", "query", "value"], 192, 192, True, id="bert"),
]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _bf16_ulp(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 7)                 # 8 significant bits


class _Attn(torch.nn.Module):
    """The call pattern of transformers' attention modules: three projections of the SAME tensor."""

    def __init__(self, Nq, Nkv, names, bias):
        super().__init__()
        self.names = names
        for n, N in zip(names, (Nq, Nkv, Nkv)):
            setattr(self, n, torch.nn.Linear(K, N, bias=bias))

    def forward(self, h):
        return tuple(getattr(self, n)(h) for n in self.names)


def _build(dev, names, targets, Nq, Nkv, bias, seed=0):
    from dalm_amd.models import lora as lora_mod

    torch.manual_seed(seed)
    m = _Attn(Nq, Nkv, names, bias).to(torch.bfloat16).to(dev)
    lora_mod.inject_lora(m, targets, r=8, lora_alpha=16, lora_dropout=0.05)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, lora_mod.LoRALinear):
                mod.lora_B["default"].weight.normal_(0, 0.1)
    return m


class _MaskSpy:
    """Records the mask bytes `lora_ops.rowdot2` made."""

    def __init__(self):
        from dalm_amd.models import lora_ops as L

        self.L, self.bits, self.orig = L, [], L.rowdot2

    def __enter__(self):
        def rowdot2(*a, **k):
            zs, bits = self.orig(*a, **k)
            self.bits += [b for b in bits if b is not None]
            return zs, bits

        self.L.rowdot2 = rowdot2
        return self

    def __exit__(self, *exc):
        self.L.rowdot2 = self.orig


def _reset_calls(m):
    from dalm_amd.models import lora as lora_mod

    for mod in m.modules():
        if isinstance(mod, lora_mod.LoRALinear):
            mod._calls = 0                                          # the same salt, hence the same masks, in every run


def _run(m, x, ups, one_gemm: bool):
    """One forward + backward; returns (outs, dx, parameter gradients, mask bytes, whether the outputs shared one storage)."""
    from dalm_amd.models import frozen_linear as FL

    old = FL._CAT
    FL._CAT = one_gemm
    try:
        for p in m.parameters():
            p.grad = None
        _reset_calls(m)
        xi = x.clone().requires_grad_(True)
        with _MaskSpy() as spy:
            outs = m(xi)
            sum((o.float() * u).sum() for o, u in zip(outs, ups)).backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        shared = len({o.untyped_storage().data_ptr() for o in outs}) == 1
        return [o.detach().clone() for o in outs], xi.grad.clone(), grads, spy.bits, shared
    finally:
        FL._CAT = old


def _float64(m, x, ups):
    from dalm_amd.models import lora as lora_mod

    x64 = x.detach().double().cpu().requires_grad_(True)
    outs, tot = [], 0.0
    for n, u in zip(m.names, ups):
        mod = getattr(m, n)
        base = mod.base_layer if isinstance(mod, lora_mod.LoRALinear) else mod
        o = x64 @ base.weight.detach().double().cpu().t()
        if base.bias is not None:
            o = o + base.bias.detach().double().cpu()
        if isinstance(mod, lora_mod.LoRALinear):
            A, Bm = (w["default"].weight.detach().double().cpu() for w in (mod.lora_A, mod.lora_B))
            o = o + mod.scaling * (x64 @ A.t()) @ Bm.t()
        outs.append(o)
        tot = tot + (o * u.double().cpu()).sum()
    tot.backward()
    return outs, x64.grad


def _inputs(dev, Nq, Nkv):
    x = torch.randn(2, R // 2, K, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)
    ups = [torch.randn(2, R // 2, N, generator=torch.Generator().manual_seed(3 + i)).bfloat16().float().to(dev)
           for i, N in enumerate((Nq, Nkv, Nkv))]
    return x, ups


@pytest.mark.parametrize("names,targets,Nq,Nkv,bias", LAYOUTS)
def test_one_forward_gemm_against_three_gemms_and_float64(dev, names, targets, Nq, Nkv, bias):
    m = _build(dev, names, targets, Nq, Nkv, bias).eval()                   # eval: no dropout, a float64 reference exists
    x, ups = _inputs(dev, Nq, Nkv)
    o3, dx3, g3, _, shared3 = _run(m, x, ups, one_gemm=False)
    o1, dx1, g1, _, shared1 = _run(m, x, ups, one_gemm=True)
    assert shared1 and not shared3                                          # one forward buffer, the outputs its slices
    assert [o.shape[-1] for o in o1] == [Nq, Nkv, Nkv]
    o64, dx64 = _float64(m, x, ups)
    for a, b, r in zip(o1, o3, o64):
        print("out: one vs three", _rel(a, b), " one vs f64", _rel(a, r), _maxerr(a, r), " three vs f64", _rel(b, r), _maxerr(b, r))
    print("dx: one vs three", _rel(dx1, dx3), " one vs f64", _rel(dx1, dx64), " three vs f64", _rel(dx3, dx64))
    for a, b, r in zip(o1, o3, o64):
        assert a.dtype == b.dtype and a.shape == b.shape and _rel(a, b) < 8e-3
        assert _rel(a, r) < 4e-3
        assert _maxerr(a, r) <= _maxerr(b, r) + _bf16_ulp(float(r.abs().max()))
    assert _rel(dx1, dx64) < 4e-3
    assert torch.equal(dx1, dx3)                                            # the same dgrad GEMMs on the same gradients
    assert sorted(g1) == sorted(g3) and len(g1) == 2 * len(targets)
    for k in g3:
        assert torch.equal(g1[k], g3[k]), k                                 # the branch reads the same g, x, z: the same bits


@pytest.mark.parametrize("names,targets,Nq,Nkv,bias", LAYOUTS)
def test_lora_gradients_and_mask_bytes_are_bit_identical_with_dropout(dev, names, targets, Nq, Nkv, bias):
    m = _build(dev, names, targets, Nq, Nkv, bias).train()                  # p = 0.05
    x, ups = _inputs(dev, Nq, Nkv)
    o3, dx3, g3, b3, _ = _run(m, x, ups, one_gemm=False)                    # the seed word is not advanced in between
    o1, dx1, g1, b1, shared1 = _run(m, x, ups, one_gemm=True)
    assert shared1
    assert len(b1) == len(b3) == len(targets) and all(int((255 - b).sum()) > 0 for b in b1)      # masks on
    for a, b in zip(b1, b3):
        assert torch.equal(a, b)
    assert sorted(g1) == sorted(g3) and len(g1) == 2 * len(targets)
    for k in g3:
        assert torch.equal(g1[k], g3[k]), k
    for a, b in zip(o1, o3):
        assert _rel(a, b) < 8e-3
    assert torch.equal(dx1, dx3)


@pytest.mark.parametrize("names,targets,Nq,Nkv,bias", LAYOUTS)
def test_slices_through_the_attention_kernels_and_a_missing_gradient(dev, names, targets, Nq, Nkv, bias):
    from dalm_amd.models import attention
    from dalm_amd.models import frozen_linear as FL

    m = _build(dev, names, targets, Nq, Nkv, bias).eval()
    x, _ = _inputs(dev, Nq, Nkv)
    B, T = x.shape[:2]

    def heads(t):
        return t.view(B, T, -1, HD).transpose(1, 2)

    def attn(q, k, v):                          # the attention kernels read the slices through their (b, h, t) strides
        return attention.sdpa(heads(q), heads(k), heads(v), None, HD ** -0.5, True).float().square().sum()

    def q_and_v_only(q, k, v):                  # k's gradient arrives as None
        return q.float().square().sum() + v.float().square().sum()

    for loss in (attn, q_and_v_only):
        dx = []
        for cat in (True, False):
            FL._CAT = cat
            try:
                xi = x.clone().requires_grad_(True)
                q, k, v = m(xi)
                assert (q.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()) == cat
                loss(q, k, v).backward()
                dx.append(xi.grad.clone())
            finally:
                FL._CAT = True
        assert bool(torch.isfinite(dx[0]).all()) and float(dx[0].abs().max()) > 0
        assert _rel(dx[0], dx[1]) < 1.2e-2


def test_state_dict_survives_and_graph_replay_matches_eager_steps(dev):
    from dalm_amd.models import frozen_linear as FL
    from dalm_amd.models import lora_ops as L

    names, targets, Nq, Nkv = ("q_proj", "k_proj", "v_proj"), ["q_proj", "v_proj"], 256, 128
    m = _build(dev, names, targets, Nq, Nkv, False).train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, ups = _inputs(dev, Nq, Nkv)
    x = x.requires_grad_(True)
    params = [p for p in m.parameters() if p.requires_grad]
    init = [p.detach().clone() for p in params]

    def step(opt):
        L.advance_dropout_seed(dev)
        _reset_calls(m)
        q, k, v = m(x)
        sum((o.float() * u).sum() for o, u in zip((q, k, v), ups)).backward()
        opt.step()

    def clear():
        x.grad = None
        for p in params:
            p.grad = None

    def restore(opt):
        """Parameters, optimizer state and the seed word as before the first step."""
        with torch.no_grad():
            for p, p0 in zip(params, init):
                p.copy_(p0)
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
        L.dropout_seed(dev).copy_(seed0)
        clear()

    seed0 = L.dropout_seed(dev).clone()
    opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
    step(opt)                                                               # the first step concatenates
    after = m.state_dict()
    assert sorted(after) == sorted(before)
    assert all(torch.equal(after[k], before[k]) for k in before if "lora_" not in k)
    ws = [m.q_proj.base_layer.weight, m.k_proj.weight, m.v_proj.base_layer.weight]
    cat = m.q_proj.base_layer._dalm_cat
    assert all(w.untyped_storage().data_ptr() == cat.untyped_storage().data_ptr() for w in ws)
    restore(opt)
    for _ in range(3):
        step(opt)
        clear()
    eager = [p.detach().clone() for p in params]

    # the same three steps replayed from a captured graph: same optimizer, same seed word, same salts
    restore(opt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                           # warm-up off the capture
        step(opt)
    torch.cuda.current_stream().wait_stream(side)
    restore(opt)
    ptrs = [w.data_ptr() for w in ws]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(opt)
    assert [w.data_ptr() for w in ws] == ptrs and m.q_proj.base_layer._dalm_cat is cat       # nothing re-pointed inside the capture
    with torch.no_grad():                                                   # the capture ran nothing; keep the captured grad buffers
        for p, p0 in zip(params, init):
            p.copy_(p0)
        for st in opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
    L.dropout_seed(dev).copy_(seed0)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for p, e, p0 in zip(params, eager, init):
        assert float((e - p0).abs().max()) > 0
        assert _rel(p.detach() - p0, e - p0) < 1e-3                        # other masks would move the Adam steps by O(1)

    assert FL.uncat_weights(m) == 1
    assert len({w.untyped_storage().data_ptr() for w in ws}) == 3
    final = m.state_dict()
    assert all(torch.equal(final[k], before[k]) for k in before if "lora_" not in k)
