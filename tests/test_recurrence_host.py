"""The recurrence grid on the CPU (tests/recurrence_cases.py): the truth is nn.LSTM's, the grid reaches every kernel at every
tile edge, the route and the launch geometry are restated, the preconditions that make the GPU test's per-unit floors
meaningful hold for every case, and the GPU test's own judging code rejects both defective formulas in every regime.

No GPU: everything here is the explicit step loop of one LSTM direction at fp64 and fp32."""
import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from tests import recurrence_cases as R

FORM_KERNEL = {"16x": "lstm16x", "16": "lstm16", "4": "lstm4", "32": "lstm32", "16s": "lstm16s", "32s": "lstm32s"}


@pytest.mark.parametrize("case", [R.Case("dprnn", 64, 1, 5, 33), R.Case("dptn", 128, 0, 4, 33, "saturated"),
                                  R.Case("dprnn", 128, 1, 17, 33, "open", bidir=False)], ids=lambda c: c.id)
def test_the_truth_is_nn_lstm_and_the_oracle(case):
    """The explicit step loop at fp64 against torch.nn.LSTM at fp64 and against oracle.dptn_oracle.lstm_direction."""
    lstm_in = R.host_lstm_input(case)
    seqs, W = R._seqs_of(case, lstm_in.a).double(), R._rnn_weights(case)
    mine = torch.cat([R.lstm_direction(seqs, W[d], d == 1) for d in range(case.ndir)], -1).numpy()
    rnn = torch.nn.LSTM(case.features, R.H, bidirectional=case.ndir == 2, batch_first=True).double()
    rnn.load_state_dict({f"{leaf}_l0{sfx}": W[d][leaf].double() for d, sfx in enumerate(("", "_reverse")[:case.ndir]) for leaf in W[d]})
    with torch.no_grad():
        theirs = rnn(seqs)[0].numpy()
    oracle = np.concatenate([O.lstm_direction(seqs.numpy(), *(W[d][k].double().numpy() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")), d == 1)
                             for d in range(case.ndir)], -1)
    a, b = R.unit_figures(mine, theirs), R.unit_figures(mine, oracle)
    print(f"{case.id}: against nn.LSTM {a[0]:.1f} dB, worst unit {a[1]:.1f}; against the oracle {b[0]:.1f} dB, worst unit {b[1]:.1f}")
    assert a[1] >= R.PIN_DB and b[1] >= R.PIN_DB
    assert np.abs(mine).max() <= 1.0 and (case.regime != "saturated" or np.abs(mine).max() > 0.99)


def test_the_grid_covers_every_kernel_at_every_tile_edge():
    """The coverage table -- (kernel, features, arch, path, edge): fewer sequences than a tile, exactly full, one over, and two
    mixtures in one tile on the strided path -- is what the geometry grid runs, no more and no less; every form runs the
    kernel it is named after, with the K4 launch everywhere but under lstm16x."""
    assert len(R.GEOMETRY_CASES) == 4 * (2 * (8 * 3 + 1) + 2 * 3 + 1) and len(R.VALUE_CASES) == 2 * 3 * 4 + 2 * 6 * 4
    assert len(set(R.CASES)) == len(R.CASES)
    assert all(c.regime == "plain" and list(R.forms(c)) == list(R.FORMS) for c in R.GEOMETRY_CASES)      # no geometry case left out
    assert {c.nseq for c in R.GEOMETRY_CASES if c.B == 1} == set(R.NSEQ) and {c.len for c in R.GEOMETRY_CASES} == {1, 2, 33, 150}
    assert all(c.nseq == 17 for c in R.CASES if c.len == 150)
    want, have = R.coverage_table(), R.grid_coverage()
    assert len(want) == 6 * 4 * 7
    assert not want - have, sorted(want - have, key=str)
    assert not have - want, sorted(have - want, key=str)
    for c in R.CASES:
        for form in R.forms(c):
            assert R.kernel_for(form, c) == FORM_KERNEL[form], (c.id, form)
            assert R.k4_launches(form, c) == (0 if form == "16x" else 1)
        assert [f for f in R.FORMS if f not in R.forms(c)] == (list(R.SPLIT_FORMS) if c.regime in R.NO_SPLIT else []), c.id
    assert len(R.LEFT_OUT) <= 2 and all(k in set(map(tuple, R.CASES)) for k in R.SEED_OVERRIDES)
    # the defaults alone: 4-sequence tiles at these sizes, which is why the 16-tile forms switch lstm4 off
    assert R.kernel_for("4", R.Case("dptn", 128, 0, 17, 33)) == "lstm4" and R.DEFAULTS["lstm4"] == 1
    # the value grid: every regime at 17 sequences, both lengths, both paths, all four (architecture, features) pairs
    for arch, f in R.ARCHS:
        for regime in (R.DPTN_REGIMES if arch == "dptn" else R.DPRNN_REGIMES):
            for path in (0, 1):
                for ln in R.VALUE_LENGTHS:
                    assert R.Case(arch, f, path, 17, ln, regime) in R.CASES


def test_tile_edges():
    e = lambda nseq, tile, **kw: R.tile_edges(R.Case("dptn", 128, kw.pop("path", 0), nseq, 2, **kw), tile)
    assert e(1, 4) == ["below"] and e(4, 4) == ["full"] and e(5, 4) == ["over"] and e(16, 4) == ["full"] and e(49, 4) == ["over"]
    assert e(5, 16) == ["below"] and e(16, 16) == ["full"] and e(17, 16) == ["over"] and e(32, 16) == ["full"] and e(49, 16) == ["over"]
    assert e(17, 32) == ["below"] and e(32, 32) == ["full"] and e(33, 32) == ["over"] and e(49, 32) == []
    assert e(9, 16, path=1, B=2) == ["spans"] and e(17, 32, path=1, B=2) == ["spans"] and e(9, 16, path=0, B=2) == []


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_launch_geometry(case):
    """Before anything runs on a device: T gives the chunk count the case names, the sequences and positions are the case's,
    the taps hold M * N and M * 256 floats, and at B = 2 on the strided path sequence 0 of the second mixture starts at
    token S * K (seq_token_base: b = q / K)."""
    g = R.stage_geometry(case)
    assert g["M"] == case.total * case.len <= 49 * 150 and g["ldh"] == 128 * case.ndir
    assert tuple(R.inputs(case).shape) == (g["B"], g["S"], g["K"], g["N"])
    assert R.host_lstm_input(case).a.shape == (g["M"], g["N"])
    seqs = R._seqs_of(case, np.arange(g["M"] * g["N"], dtype=np.float32).reshape(g["M"], g["N"]))
    assert tuple(seqs.shape) == (case.total, case.len, g["N"])
    q = case.total - 1
    base = q * g["K"] if case.path == 0 else (q // g["K"]) * g["S"] * g["K"] + q % g["K"]
    stride = 1 if case.path == 0 else g["K"]
    assert seqs[q, case.len - 1, 0] == (base + (case.len - 1) * stride) * g["N"]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_preconditions_hold(case):
    """The restatements at their bars (k32: 115 dB, 85 dB for loud and mixed; split: 88 dB) and either defect at the lowest
    floor of the case - 10 dB or below."""
    f = R.check_preconditions(case)
    print(case.id, " ".join(f"{k} {v:.1f}" for k, v in f.items()))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_the_judging_code_fails_both_defects(case):
    """The tests can fail: either defective formula, handed to the GPU test's judging code in place of a kernel result,
    misses the floor of every form; each form's restatement handed to it passes."""
    lstm_in = R.host_lstm_input(case)
    refs = R.references(case, lstm_in)
    for form, floor in R.floors(case, refs).items():
        for d in R.DEFECTS:
            if d == "row" and case.len == 1:
                continue
            with pytest.raises(AssertionError, match="worst unit"):
                R.judge(f"{form} {d}", R.defective(case, lstm_in, d), refs["truth"], floor)
        R.judge(form, refs[R.restatement_for(form)], refs["truth"], floor)
    bad = np.array(refs["truth"])
    bad[-1, -1] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        R.judge("nan", bad, refs["truth"], 0.0)


def test_the_regimes_are_what_they_say():
    """saturated reaches |h| > 0.99; open drives tanh(c) to its rail; loud overflows exp2 in fp32 and the restatement
    stays finite; quiet for DPTN (W_ih x 1e-4) and for DPRNN (x x 1e-4) keep the gates within 1e-2 of their bias."""
    for arch, f in R.ARCHS:
        c = R.Case(arch, f, 1, 17, 33, "saturated")
        assert np.abs(R.references(c, R.host_lstm_input(c))["truth"]).max() > 0.99
        c = R.Case(arch, f, 1, 17, 150, "open")
        seqs, W = R._seqs_of(c, R.host_lstm_input(c).a).double(), R._rnn_weights(c)
        h, cell = R.lstm_direction(seqs, W[0], False, cells=True)
        plain = R.Case(arch, f, 1, 17, 150)
        cell0 = R.lstm_direction(R._seqs_of(plain, R.host_lstm_input(plain).a).double(), R._rnn_weights(plain)[0], False, cells=True)[1]
        # the cell accumulates: |c| grows past 10 (tanh(c) at its rail, |h| > 0.99), where the plain weights keep it below 3
        assert cell.abs().max() > 10 and h.abs().max() > 0.99 and cell0.abs().max() < 3, (cell.abs().max(), cell0.abs().max())
        c = R.Case(arch, f, 1, 17, 33, "quiet")
        seqs, W = R._seqs_of(c, R.host_lstm_input(c).a), R._rnn_weights(c)
        assert (seqs.reshape(-1, f) @ W[0]["weight_ih"].t()).abs().max() < 1e-2
    for f in (64, 128):
        c = R.Case("dprnn", f, 1, 17, 33, "loud")
        seqs, W = R._seqs_of(c, R.host_lstm_input(c).a), R._rnn_weights(c)
        assert torch.isinf(torch.exp2((seqs.reshape(-1, f) @ W[0]["weight_ih"].t()) * -R.LOG2E)).any()
        assert all(np.isfinite(v).all() for v in R.references(c, R.host_lstm_input(c)).values())
        c = R.Case("dprnn", f, 0, 17, 33, "silent")
        assert not R.inputs(c)[0, -1].any() and np.abs(R.references(c, R.host_lstm_input(c))["truth"][-33:]).min() > 0
        c = R.Case("dprnn", f, 1, 17, 33, "mixed")
        peak = np.abs(R._seqs_of(c, R.host_lstm_input(c).a).numpy()).max(axis=(1, 2))
        assert peak[0] < 1e-2 and peak[6] > 1e3 and peak[7] < 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# training forward and BPTT
# ---------------------------------------------------------------------------------------------------------------------
def test_the_training_grid():
    """5, 16, 17, 33 sequences at 2 and 33 positions on both paths, 150 positions once per architecture; plain, saturated, open
    (and loud for DPRNN) at 17 sequences; DPTN-128, DPTN-64, DPRNN-64; both training forms.  Left out by name: DPTN x saturated
    for both forms -- the two (form, regime) pairs the grid may drop -- and nothing else."""
    assert R.TRAIN_FORMS == {"16": 1, "32": 0} and all(R.FORMS[f].get("lstm16", 1) == v for f, v in R.TRAIN_FORMS.items())
    assert len(R.TRAIN_LEFT_OUT) == 2 and set(R.TRAIN_LEFT_OUT) == {(f, "saturated") for f in R.TRAIN_FORMS}
    assert len(R.TRAIN_CASES) == len(set(R.TRAIN_CASES)) == 2 * (2 * 2 * (4 + 1) + 1) + (2 * 2 * (4 + 3) + 1)
    for arch, f in R.TRAIN_ARCHS:
        mine = [c for c in R.TRAIN_CASES if c[:2] == (arch, f)]
        assert sum(c.len == 150 for c in mine) == 1
        for path in (0, 1):
            for ln in (2, 33):
                for nseq in (5, 16, 17, 33):
                    assert R.Case(arch, f, path, nseq, ln) in mine
                for regime in R.train_regimes(arch)[1:]:
                    assert (R.Case(arch, f, path, 17, ln, regime) in mine) == (not (arch == "dptn" and regime == "saturated"))
    assert all(c.bidir and c.B == 1 for c in R.TRAIN_CASES)
    assert all(k in set(map(tuple, R.TRAIN_CASES)) for k in R.TRAIN_SEED_OVERRIDES)
    # the route of the training step: lstm_use16 alone (no lstm4, no lstm16x, no split under training)
    for c in R.TRAIN_CASES:
        assert (R.kernel_for("16", c), R.kernel_for("32", c)) == ("lstm16", "lstm32")


@pytest.mark.parametrize("case", R.TRAIN_CASES, ids=lambda c: c.id)
def test_training_preconditions_hold(case):
    """DPTN: the smallest ReLU input is >= MIN_RELU_INPUT in fp64; the fp64 reference is finite; the floors are finite, at most
    80 / 70 dB and at least 60 dB (a floor below that would judge little: the lowest, loud, is 62 dB)."""
    f = R.check_train_preconditions(case)
    print(case.id, " ".join(f"{k} {v:.3g}" for k, v in f.items()))
    floors = R.train_floors(case)
    assert all(60.0 <= v <= (80.0 if k in ("y", "dx") else 70.0) for k, v in floors.items()), floors
    if case.regime != "loud":
        assert floors["y"] == 80.0 and floors["dx"] == 80.0 and all(floors[leaf] == 70.0 for leaf in R.RNN_LEAVES), floors


@pytest.mark.parametrize("features", [128, 64])
@pytest.mark.parametrize("path", [0, 1])
def test_no_seed_meets_the_relu_precondition_for_dptn_saturated(path, features):
    """Why DPTN x saturated is left out of the training grid: at every one of the seeds a search would try, hundreds of the
    values of h that meet the ReLU lie below MIN_RELU_INPUT in fp64 (gates at their rail), and the smallest |tanh(c)| lies below it too."""
    from tests.train_attention_cases import MIN_RELU_INPUT
    for seed in range(0, R.TRAIN_SEED_LIMIT, 4):
        h, tc, below = R.saturated_relu_inputs(features, path, seed)
        print(f"dptn{features} path {path} saturated, seed {seed}: smallest |h| {h:.3g}, smallest |tanh(c)| {tc:.3g}, {below} |h| below {MIN_RELU_INPUT}")
        assert h < MIN_RELU_INPUT and tc < MIN_RELU_INPUT and below >= 100
