"""`dalm_lora_{rowdot,rankupd,colacc}` (dalm_amd/csrc/lora.hip) and the fused LoRA Linear built on them, against the eager
branch peft evaluates for the reference (dalm/models/rag_e2e_base_model.py:145-160: r = 8, alpha = 16, dropout 0.05):
    out = W x + s * B(A(dropout(x)))
* p = 0: outputs and all gradients against a float64 evaluation of that formula (f32: 2e-6 relative; bf16 tensors: the
  branch is accumulated in f32 and rounded once, so it is at least as close to float64 as the eager bf16 chain is).
* p > 0: the mask is never stored, three kernels regenerate it - adjoint identities <L x, u> = <x, L^T u> prove that forward,
  dx and dA saw the SAME mask; keep rate and rescaling are checked statistically; the seed word changes the mask."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


SHAPES = [(4608, 4096, 4096, 8), (150 * 50, 1024, 1024, 8), (37, 64, 40, 8), (5, 4104, 8200, 8), (300, 96, 72, 16), (1, 8, 8, 16),
          (9, 96, 64, 16)]     # rank 16 on the matrix cores in both weight layouts (K and N multiples of 32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,K,N,rank", SHAPES)
def test_kernels_vs_float64(dev, R, K, N, rank, dtype):
    from dalm_amd.models import lora_ops as L

    g = torch.Generator().manual_seed(R + K + N)
    x = torch.randn(R, K, generator=g).to(dtype)
    y = torch.randn(R, N, generator=g).to(dtype)
    A = torch.randn(rank, K, generator=g) / K ** 0.5
    Bm = torch.randn(N, rank, generator=g) / rank ** 0.5
    xd, yd, Ad, Bd = (t.to(dev) for t in (x, y, A, Bm))
    x64, y64, A64, B64 = (t.double() for t in (x, y, A, Bm))
    tol = 2e-6
    # rowdot, both weight layouts (bf16 rows with K % 32 == 0 run on the matrix cores with W split into bf16 high + low parts)
    tol_rd = tol if dtype == torch.float32 else 2e-5
    z = L._rowdot(xd, Ad, True, rank, 1.5, 0.0, None, 0)
    assert _rel(z, 1.5 * x64 @ A64.t()) < tol_rd
    dz = L._rowdot(yd, Bd, False, rank, 2.0, 0.0, None, 0)
    assert _rel(dz, 2.0 * y64 @ B64) < tol_rd
    # colacc, both output layouts
    db = L._colacc(yd, z, rank, 2.0, 0.0, None, 0, False)
    assert _rel(db, 2.0 * y64.t() @ z.double().cpu()) < tol
    da = L._colacc(xd, dz, rank, 1.0, 0.0, None, 0, True)
    assert _rel(da, dz.double().cpu().t() @ x64) < tol
    # rankupd, both weight layouts (result rounded once to the tensor dtype)
    rt = 1e-6 if dtype == torch.float32 else 4e-3
    out = L._rankupd_(yd.clone(), z, Bd, True, rank, 2.0, 0.0, None, 0)
    assert _rel(out, y64 + 2.0 * z.double().cpu() @ B64.t()) < rt
    dx = L._rankupd_(xd.clone(), dz, Ad, False, rank, 0.5, 0.0, None, 0)
    assert _rel(dx, x64 + 0.5 * dz.double().cpu() @ A64) < rt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,K,rank", [(4608, 4096, 8), (333, 1024, 8), (64, 8200, 8), (200, 96, 16),
                                      (9, 40, 16)])     # rank 16 off the matrix cores for bf16 rows too (K % 32 != 0)
def test_dropout_mask_is_the_same_in_all_three_kernels(dev, R, K, rank, dtype):
    """bf16 rows take the matrix-core rowdot (K % 32 == 0) and the VALU rankupd / colacc: three different code paths that have
    to agree on every mask bit."""
    from dalm_amd.models import lora_ops as L

    # small-integer data and p = 0.5 (rescale 2): every product and sum is an exact integer in bf16 / f32 / the MFMA
    # accumulator, so the adjoint identities hold EXACTLY if - and, for all practical purposes, only if - the three kernels
    # kept the same elements
    g = torch.Generator().manual_seed(R + K)
    x = torch.randint(-2, 3, (R, K), generator=g).to(dtype).to(dev)
    A = torch.randint(-1, 2, (rank, K), generator=g).float().to(dev)
    u = torch.randint(-1, 2, (R, rank), generator=g).float().to(dev)
    seed = L.dropout_seed(dev)
    salt = 1234
    z = L._rowdot(x, A, True, rank, 2.0, 0.5, seed, salt)                                        # L x
    dx = L._rankupd_(torch.zeros(R, K, device=dev), u, A, False, rank, 2.0, 0.5, seed, salt)     # L^T u
    da = L._colacc(x, u, rank, 2.0, 0.5, seed, salt, True)                                       # d <L x, u> / dA
    lhs = float((z.double() * u.double()).sum())
    assert lhs == float((x.double() * dx.double()).sum())
    assert lhs == float((A.double() * da.double()).sum())
    assert float(z.abs().sum()) > 0
    # the other weight layout of each kernel (the transposed matrix: the same products in the same order) and rankupd on a tensor
    # of the activation dtype (|dx| <= 2 * rank: exact in bf16) draw the same mask
    At = A.t().contiguous()
    assert torch.equal(L._rowdot(x, At, False, rank, 2.0, 0.5, seed, salt), z)
    assert torch.equal(L._rankupd_(torch.zeros(R, K, device=dev), u, At, True, rank, 2.0, 0.5, seed, salt), dx)
    for w, cmajor in ((A, False), (At, True)):
        dxt = L._rankupd_(torch.zeros(R, K, device=dev, dtype=dtype), u, w, cmajor, rank, 2.0, 0.5, seed, salt)
        assert torch.equal(dxt.float(), dx)
    p = 0.05
    # keep rate: with A = ones and x = ones, z (1 - p) counts the survivors of each row
    ones = torch.ones(R, K, device=dev, dtype=dtype)
    cnt = L._rowdot(ones, torch.ones(rank, K, device=dev), True, rank, 1.0, p, seed, salt)[:, 0]
    rate = float(cnt.sum()) / (R * K)
    assert abs(rate - (1 - p)) < 4 * (p * (1 - p) / (R * K)) ** 0.5 + 1e-4, rate
    # another salt, and an advanced seed word, give other masks; the same (seed, salt) gives the same one
    again = L._rowdot(ones, torch.ones(rank, K, device=dev), True, rank, 1.0, p, seed, salt)[:, 0]
    assert torch.equal(again, cnt)
    other = L._rowdot(ones, torch.ones(rank, K, device=dev), True, rank, 1.0, p, seed, salt + 1)[:, 0]
    assert not torch.equal(other, cnt) or K < 64
    L.advance_dropout_seed(dev)
    moved = L._rowdot(ones, torch.ones(rank, K, device=dev), True, rank, 1.0, p, seed, salt)[:, 0]
    assert not torch.equal(moved, cnt) or K < 64


def _record_measured(key, values):
    """Measured errors -> gpurun_out/measured_tolerances.json (the bounds in this file are stated from them)."""
    import json
    from pathlib import Path

    try:
        path = Path(__file__).resolve().parent.parent / "gpurun_out" / "measured_tolerances.json"
        path.parent.mkdir(exist_ok=True)
        cur = json.loads(path.read_text()) if path.exists() else {}
        cur[key] = values
        path.write_text(json.dumps(cur, indent=1))
    except OSError:
        pass


class _LinearSubclass(torch.nn.Linear):
    """Not `type(...) is nn.Linear`: LoRALinear must run it as its own module and add only the low-rank branch (the route nf4
    bases take as well)."""


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast", "bf16-weights-autocast", "fp32-subclass", "bf16-autocast-subclass"])
def test_fused_lora_linear_matches_the_eager_branch(dev, mode):
    """LoRALinear through lora_ops (the GPU default) against the same module with DALM_LORA_KERNEL=0 semantics (its eager
    branch), dropout off: outputs, dx, dA, dB."""
    from dalm_amd.models import lora as lora_mod

    torch.manual_seed(0)
    K, N, R = 1024, 768, 300
    base = torch.nn.Linear(K, N, bias=True)
    cls = _LinearSubclass if mode.endswith("subclass") else torch.nn.Linear
    mode = mode.replace("-subclass", "")
    mods = []
    for fused in (False, True):
        b = cls(K, N, bias=True)
        b.load_state_dict(base.state_dict())
        if mode == "bf16-weights-autocast":
            b = b.to(torch.bfloat16)
        b.requires_grad_(False)
        m = lora_mod.LoRALinear(b.to(dev), r=8, lora_alpha=16, lora_dropout=0.05).eval()     # eval: dropout off
        mods.append(m)
    mods[1].load_state_dict(mods[0].state_dict())
    with torch.no_grad():
        for m in mods:
            m.lora_B["default"].weight.copy_(torch.randn(N, 8, generator=torch.Generator().manual_seed(1)) * 0.1)
    x = torch.randn(4, R // 4, K, generator=torch.Generator().manual_seed(2)).to(dev)
    up = torch.randn(4, R // 4, N, generator=torch.Generator().manual_seed(3)).to(dev)
    res = []
    for m, fused in zip(mods, (False, True)):
        lora_mod._FUSED = fused
        try:
            xi = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
                out = m(xi)
            (out.float() * up).sum().backward()
            res.append((out.detach().float(), xi.grad.float(), m.lora_A["default"].weight.grad.float(),
                        m.lora_B["default"].weight.grad.float()))
        finally:
            lora_mod._FUSED = True
    # measured on the MI355X (profiles/r05_measured_tolerances.json): fp32 <= 3.5e-7, bf16 autocast <= 2.85e-3 (the kernels keep
    # z = A x in f32 where the eager branch rounds it to bf16); bounds = 5 x measured
    tol = 1.8e-6 if mode == "fp32" else 1.4e-2
    got = {name: _rel(a, b) for name, a, b in zip(("out", "dx", "dA", "dB"), res[1], res[0])}
    _record_measured("lora_linear:" + mode, got)
    for name, e in got.items():
        assert e < tol, f"{name}: {e:.2e}"
    assert res[1][0].dtype == res[0][0].dtype


def test_training_mode_draws_new_masks_per_step_and_backward_sees_the_forward_mask(dev):
    from dalm_amd.models import lora as lora_mod
    from dalm_amd.models import lora_ops as L

    torch.manual_seed(0)
    base = torch.nn.Linear(256, 256, bias=False).to(dev).requires_grad_(False)
    with torch.no_grad():
        base.weight.zero_()                                   # only the low-rank branch is left
    m = lora_mod.LoRALinear(base, r=8, lora_alpha=16, lora_dropout=0.5).train()
    with torch.no_grad():
        m.lora_B["default"].weight.normal_()
    x = torch.ones(64, 256, device=dev, requires_grad=True)
    outs = []
    for _ in range(2):
        L.advance_dropout_seed(dev)
        out = m(x)
        outs.append(out.detach().clone())
        x.grad = None
        out.sum().backward()
        # d out.sum() / dx[r, k] = mask[r, k] / (1 - p) * sum_c (s B A)[c, k]: zero exactly where the forward dropped x[r, k]
        col = (m.scaling * m.lora_B["default"].weight @ m.lora_A["default"].weight).sum(0)          # [K]
        mask = (x.grad / (col / 0.5)).round()
        assert set(mask.unique().tolist()) <= {0.0, 1.0}
        z_ref = (mask * x.detach() / 0.5) @ m.lora_A["default"].weight.t()
        ref = m.scaling * z_ref @ m.lora_B["default"].weight.t()
        torch.testing.assert_close(out.detach(), ref, rtol=1e-4, atol=1e-4)
        assert 0.4 < float(mask.mean()) < 0.6
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_every_mask_bit_of_every_kernel_equals_the_numpy_restatement(dev, dtype, p):
    """oracle/lora_mask.py restates the mask function in numpy integer arithmetic.  Each kernel is driven with powers of two so
    that its output spells the mask of a whole [128, 128] activation in binary: rowdot (VALU for f32, matrix cores for bf16)
    sums 2^(k % 16) over 16-column groups, colacc sums 2^(row % 16) over 16-row groups, rankupd writes the mask itself."""
    import lora_mask as O

    from dalm_amd.models import lora_ops as L

    R = K = 128
    rank = 8
    seed = L.dropout_seed(dev)
    L.advance_dropout_seed(dev)
    salt = 0xBEEF01
    want = O.keep_mask(int(seed.item()), salt, R, K, p)
    pow2 = (2.0 ** (torch.arange(K) % 16)).to(dtype)
    group = torch.arange(K) // 16                                                   # 8 groups of 16 -> the 8 rank slots

    # rankupd: y = 0 + 1 * mask * sum_j 1 * 1
    y = L._rankupd_(torch.zeros(R, K, device=dev, dtype=dtype), torch.ones(R, rank, device=dev),
                    torch.ones(rank, K, device=dev), False, rank, 1.0, p, seed, salt)
    assert np.array_equal((y.float() > 0).cpu().numpy(), want)

    # rowdot: z[row, j] = sum over the 16 columns of group j of mask * 2^(k % 16)
    x = pow2.unsqueeze(0).expand(R, K).contiguous().to(dev)
    A = (group.unsqueeze(0) == torch.arange(rank).unsqueeze(1)).float().to(dev)       # [rank, K]
    z = L._rowdot(x, A, True, rank, 1.0, p, seed, salt).cpu().numpy().astype(np.int64)   # [R, rank], exact integers < 2^16
    got = np.zeros((R, K), dtype=bool)
    for k in range(K):
        got[:, k] = (z[:, k // 16] >> (k % 16)) & 1
    assert np.array_equal(got, want)

    # colacc: out[j, c] = sum over the 16 rows of group j of mask * 2^(row % 16)
    xr = (2.0 ** (torch.arange(R) % 16)).to(dtype).unsqueeze(1).expand(R, K).contiguous().to(dev)
    zsel = ((torch.arange(R) // 16).unsqueeze(1) == torch.arange(rank).unsqueeze(0)).float().to(dev)   # [R, rank]
    out = L._colacc(xr, zsel, rank, 1.0, p, seed, salt, True).cpu().numpy().astype(np.int64)             # [rank, K]
    got = np.zeros((R, K), dtype=bool)
    for r in range(R):
        got[r, :] = (out[r // 16, :] >> (r % 16)) & 1
    assert np.array_equal(got, want)
    assert abs(want.mean() - (1 - p)) < 0.02
