"""The persistent form of the fused attention block (attn_block2.hip, option attn_persist) against one workgroup per sequence.

Nothing in a sequence's arithmetic changes -- the persistent workgroups run the same statements per sequence, take sequences by
ticket and request the next sequence's first h block ahead -- so the bar is bitwise equality of both outputs, for the default grid
(attn_persist = 1: min(sequences, CUs) workgroups) and for grids of 3 and 7 workgroups: with 3 every workgroup loops many times and
the last turns are uneven, with 7 the number of sequences is no multiple of the grid.  Shapes: the intra-chunk length stays 150
(five key blocks); the inter-chunk length = number of chunks picks the kernel's template (1..5 key blocks; from 4 on the prologue
runs its three-buffer schedule), so it is put on both sides of 32, 64, 96 and 128."""
import pytest
import torch

from speech_separation_amd.spec import DPTN_AV, DPTNConfig, synthetic_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu


def with_blocks(cfg, n):
    return DPTNConfig(**{**cfg.to_dict(), "num_blocks": n})


CFG = with_blocks(DPTN_AV, 2)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from speech_separation_amd.engine import DptnEngine, params_to_device
    dev = torch.device("cuda:0")
    e = DptnEngine(CFG, dev)
    e.bind(params_to_device(synthetic_state_dict(CFG, seed=0), dev))
    return e


def samples_for_chunks(eng, S):
    """The largest T with eng.chunks(T) == S (the number of chunks does not fall when T grows; the smallest T that counts as one
    chunk is shorter than a chunk and no supported shape)."""
    lo, hi = 16, 64000
    assert eng.chunks(hi) > S
    while lo < hi:      # the smallest T with more than S chunks
        mid = (lo + hi) // 2
        if eng.chunks(mid) > S:
            hi = mid
        else:
            lo = mid + 1
    assert eng.chunks(lo - 1) == S, f"no T gives {S} chunks"
    return lo - 1


def inputs(B, T, seed):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_inputs(CFG, B=B, T=T, Tv=50, seed=seed).items()}
    return t["mix"], t["s1_embedding"], t["s2_embedding"]


def forward(eng, persist, args):
    eng.set_option("attn_persist", persist)
    try:
        return tuple(x.clone() for x in eng.forward(*args))
    finally:
        eng.set_option("attn_persist", 1)


def check_all_grids(eng, B, T, seed):
    args = inputs(B, T, seed)
    ref = forward(eng, 0, args)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    for persist in (1, 3, 7):
        got = forward(eng, persist, args)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), f"attn_persist = {persist} differs (B = {B}, T = {T})"


@pytest.mark.parametrize("B,T", [(3, 6000), (2, 4001)], ids=["small", "ragged"])
def test_persistent_attention_block_is_bit_identical(eng, B, T):
    check_all_grids(eng, B, T, seed=31)


def test_single_chunk_leaves_workgroups_without_a_ticket(eng):
    """B = 1, one chunk: the intra-chunk launch has ONE sequence, the inter-chunk one 150 sequences of one position."""
    T = samples_for_chunks(eng, 1)
    check_all_grids(eng, 1, T, seed=32)


@pytest.mark.parametrize("S", [32, 33, 64, 65, 96, 97, 128, 129])
def test_every_key_block_count_of_the_inter_chunk_path(eng, S):
    """Inter-chunk sequences of S positions: S = 32 k is the last full key block, 32 k + 1 the first length of the next template."""
    T = samples_for_chunks(eng, S)
    assert eng.chunks(T) == S
    check_all_grids(eng, 1, T, seed=33 + S)


def test_repeated_forwards_agree(eng):
    """Three forwards under attn_persist = 1: a ticket counter that is not reset between launches shows up here."""
    args = inputs(3, 6000, seed=34)
    ref = forward(eng, 0, args)
    for _ in range(3):
        got = forward(eng, 1, args)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
