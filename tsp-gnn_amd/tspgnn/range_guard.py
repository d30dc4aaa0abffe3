"""The f16x2 range guard: four int32 words on the device and the host latches that answer them.  It decides whether a
batch, a training step or a captured graph runs on the default arithmetic or is repeated on bf16x3.

  word      byte  meaning                                                             written by
  0 flags   0     bit 0: an f16x2 operand at or beyond fp16's largest value           the f16x2 kernels (tasks' range_flag)
                  bit 1: a gate row under the variance floor                          the same
                  bit 2: replicas need a broadcast                                    Session.train_step, via the bucket
  1 weight  4     IEEE bits of max |2^s W| over the f16x2 packings since last zeroed  tspgnn_pack_weights_h2, _pack_mlp_h2
  2 status  8     a bounded wait of tspgnn_mp_loop_h2 / tspgnn_mp_resident_h2 expired those kernels
  3         12    unused

Any non-zero word 0 makes tspgnn_adam_clip_step_f32 skip.  The word-level methods are tensor operations: they work on a
CPU store too (the gloo tests).
"""
import contextlib
from collections import namedtuple

import torch

ACTIVATION, RESYNC = 3, 4           # word 0: bits 0 | 1 (an f16x2 launch left its range: repeat on bf16x3) and bit 2
WEIGHT_LIMIT_BITS = 0x46ffe000      # 32752.0f: HALF of fp16's largest finite value -- margin for the steps a training
                                    # run takes between two looks at the word (Adam moves a weight by ~lr)
BUCKET_SLOTS = (7, 8, 9)            # the data-parallel bucket's tail slots of bits 0, 1, 2 of word 0 (tspgnn_bucket_pack_f32)

Words = namedtuple("Words", "activation resync weight_over status")


def flag_bits(flags):
    """Word 0 -> (activation bits 0 / 1 / 2 / 3, replicas need a broadcast)."""
    return flags & ACTIVATION, bool(flags & RESYNC)


def decode(words):
    """A host copy of the words (a list or a pinned tensor; the first three count) -> Words(activation bits, resync, the
    weight word is at or beyond the limit, loop status)."""
    return Words(*flag_bits(int(words[0])), int(words[1]) >= WEIGHT_LIMIT_BITS, int(words[2]))


class RangeGuard(object):
    def __init__(self, store):
        self.store = store
        self.words = torch.zeros(4, dtype=torch.int32, device=store.device)   # (at finalize: not in a capture)
        self.packs_pending = 0      # f16x2 weight packings enqueued since the weight word was last taken
        self._vetoed_at = None      # store.assignments at which the variables were found outside the f16x2 range
        self._forced_off = False

    def flag_ptr(self):
        return self.words.data_ptr()

    def weight_ptr(self):
        self.packs_pending += 1     # (taken for a packing about to be enqueued)
        return self.words.data_ptr() + 4

    def status_ptr(self):
        return self.words.data_ptr() + 8

    def can_look(self):
        """A device to read from and no HIP graph being captured (a captured sequence is checked by its replay closure)."""
        return self.words.is_cuda and not torch.cuda.is_current_stream_capturing()

    def take_flags(self):
        """Word 0, cleared if set: one blocking 4-byte read."""
        flags = int(self.words[0].item())
        if flags:
            self.words[0:1].zero_()
        return flags

    def take_weight(self):
        """The weight word's bits; the word is zeroed and no packing is pending any more: one blocking 4-byte read."""
        bits = int(self.words[1].item())
        self.words[1:2].zero_()
        self.packs_pending = 0
        return bits

    def vet_weights(self, latch=True):
        """take_weight(): True if the packings stayed under the limit; if not and ``latch``, the variables are vetoed."""
        ok = self.take_weight() < WEIGHT_LIMIT_BITS
        if latch and not ok:
            self.veto()
        return ok

    def peek(self):
        """decode() of the words as they are (one blocking read); nothing is cleared."""
        return decode(self.words[:3].tolist())

    def arm(self, resync):
        """Before a training step: word 0 holds the resync bit or nothing (a stale flag would make the optimiser skip)."""
        self.words[0:1].fill_(RESYNC if resync else 0)

    def clear_flags(self):
        self.words[0:1].zero_()

    def clear_status(self):
        self.words[2:3].zero_()

    def clear(self):
        self.words.zero_()

    # -- the data-parallel bucket's tail: every rank must skip / repeat the step together (the CPU paths' arithmetic)
    def flags_to_bucket(self, tail):
        for k, slot in enumerate(BUCKET_SLOTS):
            tail[slot:slot + 1].copy_((self.words[0:1] >> k) & 1)

    def flags_from_bucket(self, tail):
        """``tail`` holds sums over the ranks: any non-zero slot sets its bit."""
        self.words[0:1].copy_(sum((tail[slot:slot + 1] != 0).to(torch.int32) << k for k, slot in enumerate(BUCKET_SLOTS)))

    # -- host latches: f16x2 is off for these variables (until they are assigned anew), or inside forced_off()
    def veto(self):
        self._vetoed_at = self.store.assignments

    def h2_off(self):
        return self._forced_off or self._vetoed_at == self.store.assignments

    @contextlib.contextmanager
    def forced_off(self):
        prev, self._forced_off = self._forced_off, True
        try:
            yield
        finally:
            self._forced_off = prev
