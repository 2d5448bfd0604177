"""CPU side of test_gpu_kws_edges.py: checks the restatements of kws_restate.py against the golden-pinned oracle, and -- on the
float64 reference alone -- every fact about the case tables and every condition on the inputs that the GPU tests rely on, so
that a GPU run is never the first place one of them fails.  The float32-arithmetic errors the GPU bounds are derived from are
re-measured here against the constants recorded in kws_restate.py, and the classifier's gradient cases are shown to notice
five mistakes a hand-written backward could make."""
import functools

import numpy as np
import pytest
import torch

import kws_restate as R
from oracle import kws_oracle as K

PIN = 1e-9                      # float64 restatement of the front-end against the float64 numpy oracle, dB; measured 2e-12


@functools.lru_cache(maxsize=None)
def _kws64(case):
    return R.kws_reference(*case)


@functools.lru_cache(maxsize=None)
def _htk64(L, n_mels, B, stretch=False):
    x = R.htk_stretch_clips() if stretch else R.htk_noise(B, L)
    return (x,) + R.htk_reference(x, n_mels, R.htk_cotangent("s" if stretch else L, x.shape[0], n_mels, x.shape[1]))


# ---- classifier ------------------------------------------------------------------------------------------------------------
def test_kws_frame_counts_are_the_cases_they_are_named_for():
    """The frame counts of the GPU tests sit where kws_kernel / kws_bwd_kernel change their trip counts, and the longest clips
    at the launcher's LDS refusal."""
    dims = {T: R.kws_dims(T) for T in R.KWS_T + (672,)}
    assert dims == {5: (1, 1), 6: (1, 1), 19: (8, 1), 20: (8, 1), 21: (9, 2), 37: (17, 3), 81: (39, 5), 672: (334, 42)}
    assert R.kws_dims(4)[0] == 0                                               # first illegal clip
    assert R.kws_dims(36)[1] == 2 and R.kws_dims(673) == (335, 42) and R.kws_dims(1001) == (499, 63)
    assert R.kws_fwd_lds_bytes(40, 64, 4, 672) == 163704 <= R.LDS_LIMIT < 163864 == R.kws_fwd_lds_bytes(40, 64, 4, 673)
    for shape in R.KWS_SHAPES:
        assert R.kws_largest_T(*shape) == R.KWS_LARGEST_T[shape]
    assert R.KWS_LARGEST_T[(60, 96, 12)] + 1 == 441 and R.KWS_LARGEST_T[(20, 128, 64)] + 1 == 437
    # the table: every T at the golden shape, every shape at 5 / 21 / 81, the longest clip of each, one clip, 300 clips
    cases = set(R.KWS_CASES)
    assert len(cases) == len(R.KWS_CASES)
    assert all(R.GOLDEN_SHAPE + (T, 8) in cases for T in R.KWS_T)
    assert all(s + (T, 8) in cases for s in R.KWS_SHAPES for T in (5, 21, 81))
    assert all(s + (R.KWS_LARGEST_T[s], 2) in cases for s in R.KWS_SHAPES)
    assert {c[4] for c in cases} == {1, 2, 8, 300}
    for n_mels, H, Kc, T, _ in R.KWS_CASES:
        assert R.kws_fwd_lds_bytes(n_mels, H, Kc, T) <= R.LDS_LIMIT
        # what ap_kws_create accepts, and the static arrays of kws_bwd_kernel (6 x 128, 2 x 128, 64)
        groups = n_mels // 20
        assert 20 <= n_mels <= 64 and H <= 128 and Kc <= 64 and n_mels % groups == 0 and H % groups == 0
    assert [s[0] // 20 for s in R.KWS_SHAPES] == [2, 1, 3, 1]
    for n_mels, H, Kc, T, _ in R.KWS_BWD_ONLY_CASES:
        assert R.kws_fwd_lds_bytes(n_mels, H, Kc, T) > R.LDS_LIMIT


@pytest.mark.parametrize("shape", R.KWS_SHAPES)
def test_kws_weights_have_the_modules_keys_at_default_init_scale(shape):
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    n_mels, H, Kc = shape
    sd, m = R.kws_weights(*shape), KWSModel(in_size=n_mels, hidden_size=H, num_classes=Kc)
    assert list(sd) == list(m.state_dict()) and all(sd[k].shape == v.shape for k, v in m.state_dict().items())
    m.load_state_dict(sd, strict=True)
    top = {k: float(v.abs().max()) for k, v in sd.items()}
    cpg = n_mels // (n_mels // 20)
    for k, fan in (("CRNN_model.sepconv.0.weight", 5), ("CRNN_model.sepconv.1.bias", cpg), ("CRNN_model.gru.weight_ih_l1", H),
                   ("CRNN_model.gru.bias_hh_l0_reverse", H), ("attn_layer.Wx_b.bias", 2 * H), ("apply_attn.U.weight", 2 * H)):
        assert 0.8 / fan ** 0.5 < top[k] <= 1.0 / fan ** 0.5 + 1e-7, (k, top[k])


@pytest.mark.parametrize("case", [R.GOLDEN_SHAPE + (81, 8), (60, 96, 12, 21, 8), (20, 128, 64, 5, 8)])
def test_unmutated_copy_of_the_forward_is_the_oracle(case):
    lp, g = _kws64(case)
    lpm, gm = R.kws_reference(*case, forward=R.kws_forward_mutable)
    assert torch.equal(lp, lpm) and torch.equal(g, gm)
    assert lp.dtype == torch.float64 and lp.shape == (case[4], case[2]) and g.shape == (case[4], case[0], case[3])


@pytest.mark.parametrize("case", R.KWS_CASES + R.KWS_BWD_ONLY_CASES)
def test_kws_reference_gradient_is_zero_exactly_off_the_read_columns(case):
    """Only frames t = 16 j + k (j < T2, k < 5) reach the model: the float64 gradient is exactly 0 elsewhere and non-zero
    somewhere in every read column.  One class: log-softmax and its gradient are identically 0."""
    n_mels, H, Kc, T, B = case
    lp, g = _kws64(case)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(g).all())
    if Kc == 1:
        assert float(lp.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
        return
    read = R.kws_read_columns(T)
    assert int(read.sum()) == min(5 * R.kws_dims(T)[1], T)
    assert bool((g[:, :, ~read] == 0.0).all())
    assert bool((g[:, :, read] != 0.0).any(dim=1).all())                       # per clip, every read column
    assert (g.abs().amax(dim=(0, 1)) > 0).tolist() == read.tolist()            # the set, derived from the gradient alone
    if T == 6:
        assert not bool(read[5])                                              # even T: the last column is in no window


def test_kws_float32_errors_are_the_recorded_ones():
    """float32 CPU evaluation of the oracle against float64 on the very cases of the GPU tests: the largest errors are the
    constants the GPU bounds are 8 x of (or the earlier bound, where that is tighter)."""
    logp = grad = 0.0
    for case in R.KWS_CASES + R.KWS_BWD_ONLY_CASES:
        lp, g = _kws64(case)
        lp32, g32 = R.kws_reference(*case, dtype=torch.float32)
        assert lp32.dtype == torch.float32
        if case in R.KWS_CASES:
            logp = max(logp, float((lp32.double() - lp).abs().max()))
        grad = max(grad, float(R.per_clip_rel_err(g32.double(), g).max()))
    print(f"float32 against float64: log-probability {logp:.2e}, gradient {grad:.2e} of max |ref|")
    assert 0 < logp <= R.REMEASURED * R.KWS_F32_LOGP_ERR
    assert 0 < grad <= R.REMEASURED * R.KWS_F32_GRAD_ERR
    assert R.KWS_LOGP_BOUND == R.GPU_FACTOR * R.KWS_F32_LOGP_ERR <= 2e-5
    assert R.KWS_GRAD_BOUND == 2e-5 < R.GPU_FACTOR * R.KWS_F32_GRAD_ERR       # the earlier bound is the tighter one


@pytest.mark.parametrize("mutate", R.KWS_MUTATIONS)
def test_gradient_cases_notice_a_mutated_backward(mutate):
    """Each mutation moves the float64 gradient by at least 50 x the GPU bound on a case of the table with enough GRU steps
    for it to matter.  Measured: detach_r 2.5e-2 to 1.1e-1, detach_zh 0.6 to 1.0, detach_attention 2.4e-2 to 8.3e-2, the
    two direction mistakes 0.3 to 1.6 of the clip's largest entry."""
    moved = {}
    for case in R.KWS_CASES:
        n_mels, H, Kc, T, B = case
        if Kc == 1 or B > 8 or R.kws_dims(T)[1] < R.KWS_MUTATION_MIN_T2[mutate]:
            continue
        _, gm = R.kws_reference(*case, forward=R.kws_forward_mutable, mutate=mutate)
        moved[case] = float(R.per_clip_rel_err(gm, _kws64(case)[1]).max())
    print(mutate, {c: f"{v:.1e}" for c, v in moved.items()})
    assert len(moved) >= 3
    assert max(moved.values()) >= R.KWS_MUTATION_FACTOR * R.KWS_GRAD_BOUND
    assert min(moved.values()) >= R.KWS_MUTATION_FACTOR * R.KWS_GRAD_BOUND     # (in fact every such case notices)


def test_kws_module_refuses_what_it_does_not_build_before_any_native_call():
    """On a CPU module a native call would raise NativeError (no CPU path): NotImplementedError comes first."""
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    with pytest.raises(NotImplementedError):
        KWSModel(kernel_size=(10, 5))
    x = R.kws_mel(40, 81, 2)
    with pytest.raises(NotImplementedError, match="inference only"):
        KWSModel().train()(x)
    with pytest.raises(NotImplementedError, match="initial GRU state"):
        KWSModel().eval()(x, hidden=torch.zeros(4, 2, 64))
    with pytest.raises(NotImplementedError, match="initial GRU state"):
        KWSModel().eval().forward(x, torch.zeros(4, 2, 64))


# ---- HTK mel-dB front-end -------------------------------------------------------------------------------------------------
def test_htk_case_table_sits_at_the_frame_count_steps():
    assert [1 + L // R.HOP for L in R.HTK_L] == [2, 2, 2, 3, 3, 3, 4, 4, 6, 81]
    cases = set(R.HTK_CASES)
    assert len(cases) == len(R.HTK_CASES)
    assert all((L, 40, R.HTK_B) in cases for L in R.HTK_L)
    assert all((L, m, R.HTK_B) in cases for m in (1, 20, 32, 64) for L in (201, 601, 16000))
    assert (1000, 40, 1) in cases and (1000, 40, 300) in cases
    assert {m for _, m, _ in cases} == set(R.HTK_MELS)
    # 201: both reflections fall on the same samples; below 400 they overlap inside one frame
    reads = R.htk_frame_samples(201)
    assert reads.shape == (2, 399) and int(reads.min()) == 0 and int(reads.max()) == 200
    assert sorted(set(reads[0].tolist())) == list(range(0, 200))
    assert sorted(set(reads[1].tolist())) == list(range(1, 201))
    for L in (201, 399):
        last = R.htk_frame_samples(L)[-1]
        assert int((last[:-1] > last[1:]).sum()) > 0 and int((last[:-1] < last[1:]).sum()) > 0
    # the reflect pad is torch's: the index table reads what F.pad(mode="reflect") holds
    for L in (201, 399, 400, 601):
        x = torch.arange(L, dtype=torch.float64)[None]
        xp = torch.nn.functional.pad(x[:, None], (200, 200), mode="reflect")[0, 0]
        assert torch.equal(xp.unfold(0, 400, 200)[:1 + L // 200, 1:].long(), R.htk_frame_samples(L))


@pytest.mark.parametrize("n_mels", R.HTK_MELS)
def test_htk_filters_are_not_empty_and_no_bin_sits_on_an_edge(n_mels):
    fb = K.mel_filterbank_htk(n_mels)
    assert fb.shape == (201, n_mels) and bool((fb.max(axis=0) > 0).all())
    assert R.htk_edge_margin(n_mels) > R.HTK_EDGE_MARGIN_HZ                    # measured 8.5e-3 Hz at 64 filters, the least
    # float32 edges (what the kernel holds) are within 2.5e-4 Hz of the float64 ones: the same bins on both sides
    pts = K.mel_to_hz_htk(np.linspace(0.0, K.hz_to_mel_htk(8000.0), n_mels + 2))
    assert float(np.abs(pts.astype(np.float32).astype(np.float64) - pts).max()) < 2.5e-4
    assert pts.astype(np.float32)[0] == 0.0 and pts.astype(np.float32)[-1] == 8000.0


@pytest.mark.parametrize("L,n_mels", [(201, 40), (601, 1), (1000, 64), (16000, 32)])
def test_htk_restatement_matches_the_oracle(L, n_mels):
    x = R.htk_noise(2, L)
    got = R.mel_htk_torch(x.double(), n_mels)
    ref = K.melspec_db_htk(x.numpy()[:, None], n_mels)[:, 0]
    assert got.shape == ref.shape == (2, n_mels, 1 + L // 200) and got.dtype == torch.float64
    assert float(np.abs(got.numpy() - ref).max()) < PIN
    assert R.mel_htk_torch(x, n_mels).dtype == torch.float32


@pytest.mark.parametrize("L,n_mels,B", R.HTK_CASES)
def test_htk_noise_cases_stay_away_from_the_clamp(L, n_mels, B):
    x, db, mel, g = _htk64(L, n_mels, B)
    assert R.htk_clamp_is_far(mel) and float(mel.min()) > 0.0                 # no silent frame: every sample has a gradient
    assert not bool(R.htk_silent_samples(mel, L).any())
    assert bool(torch.isfinite(g).all()) and bool((g != 0.0).all())


@pytest.mark.parametrize("n_mels", R.HTK_MELS)
def test_htk_stretch_clips_hold_silent_frames_and_exact_zeros(n_mels):
    """A silent frame (reflections included) has mel power exactly 0, hence exactly -100 dB; the samples only silent frames
    read have a gradient of exactly 0, and that set is the zero set of the float64 gradient."""
    L = R.HTK_STRETCH_L
    x, db, mel, g = _htk64(L, n_mels, len(R.HTK_STRETCHES), True)
    assert L == 4 * R.HTK_STRETCH and x.shape == (3, L) and float(x[2].abs().max()) == 0.0
    assert R.htk_clamp_is_far(mel)                                             # measured: the least non-zero power is 2.8e-7
    silent = R.htk_silent_frames(mel)
    assert silent.int().tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], [1] * 13]
    assert bool((db.transpose(1, 2)[silent] == -100.0).all()) and bool((db.transpose(1, 2)[~silent] > -80.0).all())
    zero = R.htk_silent_samples(mel, L)
    assert zero.sum(dim=1).tolist() == [801, 201, 2400]
    assert torch.equal(zero, g == 0.0) and bool(torch.isfinite(g).all())
    # the gradient scales as 1 / power: the quiet stretch dwarfs the loud one, which only a local scale looks at
    quiet, loud = g[0, 700:1100].abs().max(), g[0, 1300:1700].abs().max()
    assert float(quiet) > 100 * float(loud) > 0


def test_htk_silent_samples_counts_reflected_reads_and_skips_the_zero_of_the_window():
    mel = torch.ones(1, 4, 2, dtype=torch.float64)                             # L = 601: frames 0 .. 3
    mel[0, 0] = 0.0
    # frame 0 reads 1 .. 199 twice and 0; frame 1 reads 1 .. 399 (position 0 of its window weighs 0)
    assert R.htk_silent_samples(mel, 601)[0].nonzero().flatten().tolist() == [0]
    mel[0, 1] = 0.0
    assert R.htk_silent_samples(mel, 601)[0].nonzero().flatten().tolist() == list(range(0, 201))
    mel = torch.ones(1, 4, 2, dtype=torch.float64)
    mel[0, 3] = 0.0                                                            # frame 3 reads 401 .. 600 and, reflected, 599 .. 401
    assert R.htk_silent_samples(mel, 601)[0].nonzero().flatten().tolist() == [600]


def test_htk_float32_errors_are_the_recorded_ones():
    """float32 CPU evaluation of the restatement against float64 on the very cases of the GPU tests."""
    db_err = grad_err = 0.0
    runs = [(c, False) for c in R.HTK_CASES] + [((R.HTK_STRETCH_L, m, 3), True) for m in R.HTK_MELS]
    for (L, n_mels, B), stretch in runs:
        x, db, mel, g = _htk64(L, n_mels, B, stretch)
        v = R.htk_cotangent("s" if stretch else L, x.shape[0], n_mels, L)
        db32, _, g32 = R.htk_reference(x, n_mels, v, dtype=torch.float32)
        assert db32.dtype == torch.float32
        db_err = max(db_err, float((db32.double() - db).abs().max()))
        scale = R.htk_local_scale(g)
        d = (g32.double() - g).abs()
        assert bool((d[scale == 0.0] == 0.0).all())
        grad_err = max(grad_err, float((d / scale.clamp(min=1e-300))[scale > 0].max()))
    print(f"float32 against float64: {db_err:.2e} dB, gradient {grad_err:.2e} of the local max |ref|")
    assert 0 < db_err <= R.REMEASURED * R.HTK_F32_DB_ERR
    assert 0 < grad_err <= R.REMEASURED * R.HTK_F32_GRAD_ERR
    assert R.HTK_DB_BOUND == R.GPU_FACTOR * R.HTK_F32_DB_ERR <= 5e-3
    assert R.HTK_GRAD_BOUND == 2e-4 < R.GPU_FACTOR * R.HTK_F32_GRAD_ERR       # the earlier figure is the tighter one
