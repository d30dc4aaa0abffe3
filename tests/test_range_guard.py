"""The f16x2 range guard's host side (tspgnn/range_guard.py) on a store finalised on the CPU: word layout, the taking
reads, the latches GraphNN.active_arith() follows, the decoding of a host copy and the data-parallel bucket's tail."""
import itertools

import numpy as np
import pytest
import torch

import tspgnn
from tspgnn import range_guard
from tspgnn import variables as V

UNDER, AT = 0x46ffdfff, 0x46ffe000      # the weight word just under and at the limit (32752.0f = half of fp16's largest)


@pytest.fixture
def model():
    m = tspgnn.build_network(32, store=V.VariableStore())
    m.store.finalize("cpu")
    m.store.initialize(seed=1)
    return m


def test_words_and_addresses_after_finalize(model):
    store, guard = model.store, model.store.guard
    words = store.h2_guard()
    assert words is guard.words and words.dtype == torch.int32 and words.tolist() == [0, 0, 0, 0]
    base = words.data_ptr()
    assert guard.flag_ptr() == base and guard.status_ptr() == base + 8 and guard.packs_pending == 0
    assert guard.weight_ptr() == base + 4 and guard.packs_pending == 1
    assert guard.flag_ptr() == base and guard.status_ptr() == base + 8 and guard.packs_pending == 1


def test_take_flags_clears_word_0_only(model):
    guard = model.store.guard
    guard.words.copy_(torch.tensor([6, 1234, 5, 0], dtype=torch.int32))
    assert guard.take_flags() == 6
    assert guard.words.tolist() == [0, 1234, 5, 0]
    assert guard.take_flags() == 0
    assert guard.words.tolist() == [0, 1234, 5, 0]


def test_take_weight_zeroes_word_1_and_the_pending_count(model):
    guard = model.store.guard
    guard.words.copy_(torch.tensor([3, UNDER, 5, 0], dtype=torch.int32))
    guard.weight_ptr(), guard.weight_ptr()
    assert guard.packs_pending == 2
    assert guard.take_weight() == UNDER
    assert guard.words.tolist() == [3, 0, 5, 0] and guard.packs_pending == 0


@pytest.mark.parametrize("assign", [lambda store: store.initialize(seed=2),
                                    lambda store: store.load({"V_init": np.ones((1, 32), dtype=np.float32)})])
def test_weight_limit_vetoes_until_the_variables_are_assigned(model, assign):
    store, guard, gnn = model.store, model.store.guard, model["gnn"]
    assert gnn.active_arith() == "h2" and not guard.h2_off()
    guard.words[1:2].fill_(UNDER)
    guard.weight_ptr()
    assert guard.vet_weights() and not guard.h2_off() and gnn.active_arith() == "h2"
    assert guard.words.tolist() == [0, 0, 0, 0] and guard.packs_pending == 0
    guard.words[1:2].fill_(AT)
    guard.weight_ptr()
    assert not guard.vet_weights() and guard.h2_off() and gnn.active_arith() == "x3"
    assert guard.words.tolist() == [0, 0, 0, 0] and guard.packs_pending == 0
    assert gnn.check_h2_weights()           # (already vetoed for these variables: the caller's plan stands)
    assign(store)
    assert not guard.h2_off() and gnn.active_arith() == "h2"
    guard.words[1:2].fill_(AT)              # the bf16-native backward's look: an answer, no veto
    assert not guard.vet_weights(latch=False) and not guard.h2_off() and gnn.active_arith() == "h2"


def test_forced_off_h2_restores_the_previous_state(model):
    gnn = model["gnn"]
    with gnn.forced_off_h2():
        assert gnn.active_arith() == "x3"
        with gnn.forced_off_h2():
            assert gnn.active_arith() == "x3"
        assert gnn.active_arith() == "x3"       # the inner block's exit restores "off", not "on"
    assert gnn.active_arith() == "h2"
    with pytest.raises(KeyError):
        with gnn.forced_off_h2():
            assert gnn.active_arith() == "x3"
            raise KeyError("inside")
    assert gnn.active_arith() == "h2"
    gnn.leave_h2()
    with gnn.forced_off_h2():
        assert gnn.active_arith() == "x3"
    assert gnn.active_arith() == "x3"           # the veto is another latch: the block's exit leaves it alone


# word 0 -> (activation bits, replicas need a broadcast)
FLAGS = {0: (0, False), 1: (1, False), 2: (2, False), 3: (3, False), 4: (0, True), 5: (1, True), 6: (2, True), 7: (3, True)}


@pytest.mark.parametrize("flags,weight,status", itertools.product(range(8), [UNDER, AT], [0, 9]))
def test_decode(flags, weight, status):
    want = FLAGS[flags] + (weight == AT, status)
    assert tuple(range_guard.decode([flags, weight, status])) == want
    got = range_guard.decode(torch.tensor([flags, weight, status, 77], dtype=torch.int32))    # (a pinned copy of all four)
    assert (got.activation, got.resync, got.weight_over, got.status) == want
    assert range_guard.flag_bits(flags) == FLAGS[flags]


# word 0 -> slots 7, 8, 9 of the bucket's tail (bits 0, 1, 2), as tspgnn_bucket_pack_f32 writes them
SLOTS = {0: [0.0, 0.0, 0.0], 1: [1.0, 0.0, 0.0], 2: [0.0, 1.0, 0.0], 3: [1.0, 1.0, 0.0],
         4: [0.0, 0.0, 1.0], 5: [1.0, 0.0, 1.0], 6: [0.0, 1.0, 1.0], 7: [1.0, 1.0, 1.0]}
# slots 7, 8, 9 summed over the ranks -> word 0, as tspgnn_bucket_unpack_f32 restores it
SUMS = [([0.0, 0.0, 0.0], 0), ([1.0, 0.0, 0.0], 1), ([0.0, 3.0, 0.0], 2), ([2.0, 1.0, 0.0], 3), ([0.0, 0.0, 4.0], 4),
        ([1.0, 0.0, 2.0], 5), ([0.0, 8.0, 1.0], 6), ([3.0, 2.0, 1.0], 7)]


@pytest.mark.parametrize("flags", range(8))
def test_bucket_tail_carries_one_slot_per_flag_bit(model, flags):
    sess = tspgnn.Session(model, device="cpu")
    store, guard = model.store, model.store.guard
    stats = torch.tensor([0.5, 0.25, 1.0, 2.0, 3.0, 4.0])
    guard.words.copy_(torch.tensor([flags, 1234, 5, 0], dtype=torch.int32))
    tail = sess._pack_bucket(4, stats, False)
    assert tail.tolist() == [4.0, 2.0, 1.0, 1.0, 2.0, 3.0, 4.0] + SLOTS[flags]
    assert guard.words.tolist() == [flags, 1234, 5, 0]
    sums, word = SUMS[flags]
    tail[0:1].fill_(8.0)
    tail[7:10].copy_(torch.tensor(sums))
    guard.words[0:1].fill_(7 - flags)           # whatever the word held, it is the tail's afterwards
    sess._unpack_bucket(stats, False)
    assert guard.words.tolist() == [word, 1234, 5, 0]
    assert stats.tolist() == [0.25, 0.125, 1.0, 2.0, 3.0, 4.0]
