"""CPU side of test_gpu_kws_train.py: every fact about the case table and every condition on the float64 reference that the GPU
tests of the KWS training step rely on, so that a GPU run is never the first place one of them fails; the float32-arithmetic
errors the GPU bounds are derived from, re-measured against the constants recorded in kws_train_restate.py; and the proof that
those bounds see four mistakes a hand-written parameter-gradient contraction could make."""
import numpy as np
import pytest
import torch

import kws_restate as R
import kws_train_restate as TR

BY_HAND = 1e-12                 # float64 hand-written backward against float64 autograd, of a tensor's largest entry; measured 1.2e-14
ALL_CASES = TR.TRAIN_CASES + TR.TRAIN_BWD_ONLY_CASES


def test_train_frame_counts_and_batches_are_the_cases_they_are_named_for():
    assert [R.kws_dims(T)[1] for T in TR.TRAIN_T] == [1, 1, 1, 2, 3, 5]
    assert R.kws_dims(20)[1] == 1 and R.kws_dims(21)[1] == 2                    # where a second GRU step appears
    cases = set(TR.TRAIN_CASES)
    assert len(cases) == len(TR.TRAIN_CASES) == 19
    assert all(R.GOLDEN_SHAPE + (T, 8) in cases for T in (5, 19, 20, 21, 37, 81))
    assert all(s + (T, 8) in cases for s in [(20, 128, 64), (60, 96, 12), (32, 8, 1)] for T in (5, 21, 81))
    assert {(40, 64, 4, 81, 1), (40, 64, 4, 81, 67), (40, 64, 4, 81, 300), (32, 64, 4, 161, 8)} <= cases
    assert (67 * R.kws_dims(81)[1]) % TR.SLICES != 0 and 67 % TR.SLICES != 0   # neither the items nor the clips split evenly
    assert TR.TRAIN_BWD_ONLY_CASES == [(40, 64, 4, 1001, 2)] and R.kws_dims(1001)[1] == 63
    for n_mels, H, Kc, T, _ in TR.TRAIN_CASES:
        assert R.kws_fwd_lds_bytes(n_mels, H, Kc, T) <= R.LDS_LIMIT
        groups = n_mels // 20
        assert 20 <= n_mels <= 64 and H <= 128 and Kc <= 64 and n_mels % groups == 0 and H % groups == 0
    assert R.kws_fwd_lds_bytes(40, 64, 4, 1001) > R.LDS_LIMIT
    assert R.kws_dims(161) == (79, 10)


def test_parameters_come_in_state_dict_order():
    """The gradient blob is split in state-dict order and handed to autograd in parameters() order: they are one order, and the
    state dict holds nothing but parameters."""
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    m = KWSModel(in_size=32)
    assert [k for k, _ in m.named_parameters()] == list(m.state_dict())
    assert list(TR.train_reference(R.GOLDEN_SHAPE + (5, 8))[2]) == list(KWSModel().state_dict())


@pytest.mark.parametrize("case", ALL_CASES)
def test_reference_gradients_are_nonzero_except_where_they_are_zero_by_construction(case):
    n_mels, H, Kc, T, B = case
    lp, dx, g = TR.train_reference(case)
    assert lp.dtype == torch.float64 and list(g) == list(R.kws_weights(n_mels, H, Kc))
    zero = [k for k in g if TR.exact_zero(k, Kc, T)]
    if Kc == 1:
        assert zero == list(g)
    elif R.kws_dims(T)[1] == 1:
        assert zero == ["CRNN_model.gru.weight_hh_l0", "CRNN_model.gru.weight_hh_l0_reverse", "CRNN_model.gru.weight_hh_l1",
                        "CRNN_model.gru.weight_hh_l1_reverse", "attn_layer.Wx_b.weight", "attn_layer.Wx_b.bias", "attn_layer.Vt.weight"]
    else:
        assert zero == []
    for k, v in g.items():
        assert v.shape == R.kws_weights(n_mels, H, Kc)[k].shape and bool(torch.isfinite(v).all())
        top = float(v.abs().max())
        if k in zero:
            assert top == 0.0, k
        else:
            assert top >= 4e-4, (k, top)                                       # measured: the least is 4.9e-4


def test_train_float32_errors_are_the_recorded_ones():
    """float32 CPU evaluation of the autograd reference against float64 on the very cases of the GPU tests; exact zeros are
    exact in float32 too."""
    worst, where = 0.0, None
    for case in ALL_CASES:
        _, _, g = TR.train_reference(case)
        _, _, g32 = TR.train_reference(case, torch.float32)
        for k in g:
            assert g32[k].dtype == torch.float32
            e = TR.tensor_rel_err(g32[k], g[k])
            if TR.exact_zero(k, case[2], case[3]):
                assert e == 0.0
            if e > worst:
                worst, where = e, (case, k)
    print(f"float32 against float64: parameter gradient {worst:.2e} of max |ref| at {where}")
    assert 0 < worst <= R.REMEASURED * TR.TRAIN_F32_GRAD_ERR
    assert TR.TRAIN_GRAD_BOUND == R.GPU_FACTOR * TR.TRAIN_F32_GRAD_ERR < 1e-4


@pytest.mark.parametrize("case", [R.GOLDEN_SHAPE + (81, 8), (60, 96, 12, 21, 8), (20, 128, 64, 5, 8), (32, 64, 4, 161, 8),
                                  (32, 8, 1, 21, 8)])
def test_unmutated_backward_by_hand_is_autograd(case):
    lp, dx, g = TR.train_reference(case)
    lph, dxh, gh = TR.by_hand(case)
    assert float((lph - lp).abs().max()) < 1e-14 and TR.tensor_rel_err(dxh, dx) < BY_HAND
    assert list(gh) == list(g)
    for k in g:
        assert gh[k].shape == g[k].shape and TR.tensor_rel_err(gh[k], g[k]) < BY_HAND, k


@pytest.mark.parametrize("mutate,moves", [
    ("hidden_n_not_scaled_by_r", ("bias_hh", "weight_hh")), ("weight_hh_with_h_t", ("weight_hh",)),
    ("reverse_pairs_mirrored_input", ("weight_ih_l0_reverse", "weight_ih_l1_reverse")), ("l1_weight_ih_forward_half", ("weight_ih_l1",))])
def test_gradient_cases_notice_a_mutated_contraction(mutate, moves):
    """Each mutation moves at least one parameter tensor by KWS_MUTATION_FACTOR x the GPU bound on every case with enough GRU steps
    for it to matter (measured: 0.6 to 2.0 of the tensor's largest entry), moves only the tensors it is about, and leaves the
    input gradient alone."""
    moved = {}
    for case in TR.TRAIN_CASES:
        n_mels, H, Kc, T, B = case
        if Kc == 1 or B > 8 or R.kws_dims(T)[1] < TR.TRAIN_MUTATION_MIN_T2[mutate]:
            continue
        _, dx, g = TR.train_reference(case)
        _, dxm, gm = TR.by_hand(case, mutate)
        errs = {k: TR.tensor_rel_err(gm[k], g[k]) for k in g}
        assert TR.tensor_rel_err(dxm, dx) < BY_HAND
        assert all(any(m in k for m in moves) for k, e in errs.items() if e >= BY_HAND), [k for k, e in errs.items() if e >= BY_HAND]
        moved[case] = max(errs.values())
    print(mutate, {c: f"{v:.1e}" for c, v in moved.items()})
    assert len(moved) >= 3
    assert min(moved.values()) >= R.KWS_MUTATION_FACTOR * TR.TRAIN_GRAD_BOUND


def test_adam_float32_error_is_the_recorded_one():
    p64, mask = TR.adam_reference()
    p32, _ = TR.adam_run(torch.float32)
    err = TR.adam_err(p32, p64, mask)
    w0 = R.kws_weights(*TR.ADAM_CASE[:3])
    step = max(float((p64[k] - w0[k].double()).abs().max()) for k in p64) / TR.ADAM_LR
    kept = sum(int(m.sum()) for m in mask.values()) / sum(m.numel() for m in mask.values())
    print(f"three Adam steps, float32 against float64: {err:.2e} lr on {kept:.0%} of the entries; largest move {step:.2f} lr")
    assert 0 < err <= R.REMEASURED * TR.ADAM_F32_ERR
    assert all(bool(m.any()) for m in mask.values()) and kept > 0.5            # every tensor is compared somewhere
    assert step > 2.5                                                          # the steps move parameters by about 3 lr: 3e3 x the bound
    assert TR.ADAM_BOUND == R.GPU_FACTOR * TR.ADAM_F32_ERR


def test_golden_file_agrees_with_the_restatement():
    """The reference's own model class in train(), CrossEntropyLoss on its log-probabilities, backward(): the oracle with autograd
    gives the same numbers in float64 (the golden file is float32: 1e-5 of a tensor's largest entry; measured below 3e-6)."""
    from oracle import kws_oracle as K
    G, W = np.load(TR.GOLDEN_TRAIN), np.load(R.ROOT + "/tests/golden/golden_kws_v1.npz")
    assert not any("/sd/" in k for k in G.files)                               # weights are not stored again
    for tag, n_mels, T, B in (("m32/T161_B3", 32, 161, 3), ("m40/T81_B1", 40, 81, 1)):
        sd = {k.split("/sd/")[1]: torch.from_numpy(W[k]).double().requires_grad_(True) for k in W.files if k.startswith(f"m{n_mels}/sd/")}
        x = TR.golden_input(n_mels, T, B).double().requires_grad_(True)
        lp = K.kws_forward(sd, x, hidden=64)
        loss = torch.nn.CrossEntropyLoss()(lp, TR.train_targets(B, 4))
        loss.backward()
        assert abs(float(loss.detach()) - float(G[f"{tag}/loss"])) < 1e-6
        assert TR.tensor_rel_err(x.grad, torch.from_numpy(G[f"{tag}/dx"])) < 1e-5
        names = [k.split("/grad/")[1] for k in G.files if k.startswith(f"{tag}/grad/")]
        assert sorted(names) == sorted(sd) if B == 3 else len(names) == 4
        for k in names:
            assert TR.tensor_rel_err(sd[k].grad, torch.from_numpy(G[f"{tag}/grad/{k}"])) < 1e-5, k
        if B == 3:
            assert float((lp.detach() - torch.from_numpy(G[f"{tag}/logp"])).abs().max()) < 2e-6


def test_cpu_module_in_train_mode_still_refuses_before_any_native_call():
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    with pytest.raises(NotImplementedError, match="no CPU training path.*inference only"):
        KWSModel().train()(R.kws_mel(40, 81, 2))
