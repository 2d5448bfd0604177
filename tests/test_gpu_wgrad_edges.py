"""ap_wgrad_corr where wgrad_corr_kernel branches: slices of three and four chunks that walk from a clip's partial last chunk
into the next clip, every remainder of a tap's 16-byte-aligned window, the scalar loads (by length and by pointer), half-empty
tiles, one chunk in one slice -- the cases of wgrad_restate.py, whose tags test_wgrad_restate_cpu.py asserts.  On integer data
the result is compared EXACTLY with the float64 einsum (any summation order gives the same integers), so one sample from the
wrong clip, one padded position that received the FiLM add or one dropped column fails; precision is what the GATE rows and
test_gpu_train.py's tolerance cases measure.  The workspace starts NaN-filled on every call: a NaN in a result is a slot the
reduction read and this call did not write."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import synth  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402
import wgrad_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def corr(dev, P, Q, film, taps, dil, mode, scale=1.0, G=None, accumulate=0):
    """One call on device tensors P [B][M][L], Q [B][N or 2N][L]: NaN-filled workspace of exactly the size asked for; G NaN-filled
    unless given."""
    lib = N.lib()
    B, M, L = P.shape
    Nn = Q.shape[1] // 2 if mode == R.GATE else Q.shape[1]
    need = lib.ap_wgrad_workspace_bytes(B, M, Nn, L, taps)
    assert need == R.workspace_bytes(B, M, Nn, L, taps) > 0
    ws = torch.full((need // 4,), NAN, device=dev)
    if G is None:
        G = torch.full((M, Nn, taps), NAN, device=dev)
    N.check(lib.ap_wgrad_corr(N.ptr(P), N.ptr(Q), N.ptr(film), N.ptr(G), ws.data_ptr(), need, B, M, Nn, L, taps, dil, mode, scale, accumulate,
                              N.stream()), "ap_wgrad_corr")
    return G


@functools.lru_cache(maxsize=None)
def _on_device(name):
    return tuple(t.cuda() for t in R.integer_inputs(name))


# ---- a. exact comparison on integer data ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dil", R.EXACT_CASES)
def test_integer_data_gives_the_exact_sum(dev, name, dil):
    """PLAIN and FILM at p_scale 1 and 0.5 from a NaN-filled G and workspace; then accumulate = 1 onto an integer prior."""
    r = R.ROWS[name]
    P, Q, film, prior = R.integer_inputs(name)
    Pd, Qd, fd, pd = _on_device(name)
    assert R.uses_vec(r.L, Pd.data_ptr(), Qd.data_ptr()) == ("scalar" not in r.tags)
    for mode in (R.PLAIN, R.FILM):
        ref = R.corr_reference(P, Q, film, r.taps, dil, mode)
        for scale in (1.0, 0.5):
            G = corr(dev, Pd, Qd, fd if mode == R.FILM else None, r.taps, dil, mode, scale).cpu().double()
            assert not torch.isnan(G).any(), "the reduction read a workspace slot this call did not write"
            bad = (G != scale * ref)
            assert torch.equal(G, scale * ref), (f"mode {mode} scale {scale}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                                 f"{bad.nonzero()[0].tolist()}, by up to {float((G - scale * ref).abs().max())}")
            for k, (_, _, _, on) in enumerate(R.tap_windows(r.taps, dil, r.L)):
                if not on:                                        # a tap no sample meets: exact zeros
                    assert float(ref[:, :, k].abs().max()) == 0.0 and torch.count_nonzero(G[:, :, k]).item() == 0
        G3 = corr(dev, Pd, Qd, fd if mode == R.FILM else None, r.taps, dil, mode, 1.0, G=pd.clone(), accumulate=1)
        assert torch.equal(G3.cpu().double(), prior.double() + ref)


def test_three_one_clip_calls_add_up_to_the_three_clip_call(dev):
    """Batch additivity on the deep row: each clip alone has another slicing (35 chunks over 32 slices), the integers are the same."""
    r = R.ROWS["deep_vec"]
    Pd, Qd, fd, _ = _on_device("deep_vec")
    for mode, dil in ((R.FILM, 5), (R.PLAIN, 1)):
        f = fd if mode == R.FILM else None
        whole = corr(dev, Pd, Qd, f, 3, dil, mode)
        acc = torch.zeros_like(whole)
        for b in range(r.B):
            corr(dev, Pd[b:b + 1], Qd[b:b + 1], f, 3, dil, mode, G=acc, accumulate=1)
        assert torch.equal(acc, whole)
        assert float(whole.abs().max()) > 0


# ---- b. GATE against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in R.GATE_ROWS])
def test_gate_mode_matches_float64_at_saturating_pre_activations(dev, name):
    """tanh times sigmoid in float64, then the einsum; the project's bar of 1e-4 max|G_ref|.  Planted +-15, +-16, +-40 (tanh half) and
    +-80, +-100 (sigmoid half): every output finite.  Measured on an MI355X: see DESIGN.md."""
    r = R.ROWS[name]
    P, Q = R.gate_inputs(name)
    dil = r.dils[0]
    ref = R.corr_reference(P, Q, None, r.taps, dil, R.GATE)
    Pd, Qd = P.to(dev), Q.to(dev)
    assert R.uses_vec(r.L, Pd.data_ptr(), Qd.data_ptr()) == ("scalar" not in r.tags)
    G1 = corr(dev, Pd, Qd, None, r.taps, dil, R.GATE)
    G2 = corr(dev, Pd, Qd, None, r.taps, dil, R.GATE, G=torch.empty_like(G1))
    assert torch.isfinite(G1).all()
    assert torch.equal(G1, G2)                                    # two runs: the same bits
    tol = 1e-4 * float(ref.abs().max())
    err = float((G1.cpu().double() - ref).abs().max())
    print(f"{name}: max|G - G_ref| = {err:.3e} = {err / float(ref.abs().max()):.3e} of max|G_ref|, bound {tol:.3e}")
    assert err <= tol


# ---- c. the alignment fallback --------------------------------------------------------------------------------------------------
def _misplaced(t):
    """a contiguous copy of t that starts one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def test_a_misaligned_operand_takes_the_scalar_loads_and_gives_the_same_bits(dev):
    """The staged values, and so the MFMA sequence, are the same by construction whichever loads fetch them."""
    r = R.ROWS["deep_vec"]
    key = "wgalign"
    P = torch.from_numpy(synth.uniform(key + "P", (r.B, r.M, r.L), 3))
    Q = torch.from_numpy(synth.uniform(key + "Q", (r.B, r.N, r.L), 3, -2.0, 2.0))
    film = torch.from_numpy(synth.uniform(key + "f", (r.N,), 3, 1.0, 3.0))
    dil, scale = 2, 0.5 ** 0.5
    ref = scale * R.corr_reference(P, Q, film, 3, dil, R.FILM)
    Pd, Qd, fd = P.to(dev), Q.to(dev), film.to(dev)
    Pm, Qm = _misplaced(Pd), _misplaced(Qd)
    assert R.uses_vec(r.L, Pd.data_ptr(), Qd.data_ptr())
    assert not R.uses_vec(r.L, Pm.data_ptr(), Qd.data_ptr()) and not R.uses_vec(r.L, Pd.data_ptr(), Qm.data_ptr())
    Gs = [corr(dev, p, q, fd, 3, dil, R.FILM, scale) for p, q in ((Pd, Qd), (Pm, Qd), (Pd, Qm))]
    tol = 1e-4 * float(ref.abs().max())
    for G in Gs:
        err = float((G.cpu().double() - ref).abs().max())
        print(f"max|G - G_ref| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol
    assert torch.equal(Gs[0], Gs[1]) and torch.equal(Gs[0], Gs[2])


# ---- d. refusals ----------------------------------------------------------------------------------------------------------------
def test_wgrad_corr_refuses_more_bad_arguments_and_writes_nothing(dev):
    lib = N.lib()
    t = torch.ones(64 * 64 * 40, device=dev)
    G = torch.full((64 * 64 * 3,), NAN, device=dev)
    ws = torch.full((1 << 18,), NAN, device=dev)
    wsb = ws.numel() * 4

    def call(M=32, Nn=32, dil=1, mode=R.PLAIN, w=ws.data_ptr(), L=40):
        return lib.ap_wgrad_corr(N.ptr(t), N.ptr(t), None, N.ptr(G), w, wsb, 1, M, Nn, L, 3, dil, mode, 1.0, 0, N.stream())

    assert call(M=0) == -22 and call(Nn=16) == -22 and call(dil=0) == -22 and call(mode=3) == -22 and call(mode=-1) == -22
    assert call(w=None) == -22
    # the range check: 2 dil + L + 64 must fit an int (the window arithmetic t0 + al + 4 q of the kernel)
    assert call(dil=R.DIL_LIMIT(40) + 1) == -22 and b"out of range" in lib.ap_last_error()
    assert call(dil=2 ** 31 - 1) == -22
    torch.cuda.synchronize()
    assert torch.isnan(G).all() and torch.isnan(ws).all()         # nothing was launched
    # the largest dilation it accepts: both outer taps off, the centre tap the plain sum
    N.check(call(dil=R.DIL_LIMIT(40)), "ap_wgrad_corr")
    g = G.view(64 * 64, 3)[:32 * 32].cpu()
    assert torch.equal(g, torch.tensor([0.0, 40.0, 0.0]).expand(32 * 32, 3))
