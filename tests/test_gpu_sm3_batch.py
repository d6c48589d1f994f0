"""ovh_sm3_batch / ovh_sm3_batch_device (k_sm3_bulk, csrc/sm3_bulk.hpp) on the device against
hashlib's SM3: block-boundary lengths, a wave with one long lane, wave tails, unaligned device
buffers, reversed offsets and the host form's argument checks."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 191, 192, 1000, 4097]


def sm3(b):
    return hashlib.new("sm3", bytes(b)).digest()


def message(n, salt=0):
    return random.Random(0xB17C + 131 * n + salt).randbytes(n)


@pytest.fixture(scope="module")
def cc():
    import consensus_overlord_amd as coa
    return coa.ConsensusCrypto(bytes.fromhex("97" * 32))


def test_lengths_and_one_long_lane(cc):
    """Every padding case, and one 70,001-byte message among short ones: its wave has one long
    lane, and after the ordering by block count, waves with lanes that end early."""
    msgs = [message(n) for n in LENGTHS]
    msgs = msgs[:7] + [message(70001)] + msgs[7:]
    assert cc.hash_batch(msgs) == [sm3(m) for m in msgs]


def test_wave_tails_and_empty_messages(cc):
    for n in (1, 63, 64, 65, 130):
        msgs = [message((37 * i) % 150, n) for i in range(n)]
        assert cc.hash_batch(msgs) == [sm3(m) for m in msgs], n
    assert cc.hash_batch([b""] * 70) == [sm3(b"")] * 70
    assert cc.hash_batch([]) == []


def test_device_form_unaligned_canary_and_reversed_offsets(cc):
    import torch
    msgs = [message(n, 3) for n in (5, 64, 129, 0, 1000, 57, 200)]
    data = b"".join(msgs)
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    # entry 3 (empty) becomes an entry whose end lies below its start: offsets ..., 198, 150, 1198
    # give entry 2 = data[69:198] as before, entry 3 reversed, entry 4 = data[150:1198]
    off_rev = list(off)
    off_rev[4] = 150
    want = [sm3(m) for m in msgs]
    want_rev = list(want)
    want_rev[3] = bytes(32)
    want_rev[4] = sm3(data[150:off[5]])
    dev = torch.device("cuda:0")
    n = len(msgs)
    for shift in (1, 2, 3):
        raw = torch.full((len(data) + 16,), 0xA5, dtype=torch.uint8)
        raw[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        d_raw = raw.to(dev)
        d_data = d_raw[shift:]                      # a device pointer `shift` bytes off alignment
        assert d_data.data_ptr() % 4 == shift
        for offsets, expect in ((off, want), (off_rev, want_rev)):
            d_off = torch.tensor(offsets, dtype=torch.int64, device=dev)
            d_out = torch.full((32 * n + 32,), 0xAA, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            code = cc.lib.ovh_sm3_batch_device(cc.ctx.ptr, n, ctypes.c_void_p(d_data.data_ptr()),
                                               ctypes.c_void_p(d_off.data_ptr()), ctypes.c_void_p(d_out.data_ptr()))
            assert code == 0
            # the kernel runs on the context's stream: wait for the device before reading
            torch.cuda.synchronize()
            out = d_out.cpu().numpy().tobytes()
            assert [out[32 * i:32 * i + 32] for i in range(n)] == expect, shift
            assert out[32 * n:] == b"\xaa" * 32, "canary after the digests"


def test_host_form_argument_checks(cc):
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    data = np.frombuffer(message(64), dtype=np.uint8)
    out = np.full(64, 0xEE, dtype=np.uint8)
    bad = np.array([0, 40, 30], dtype=np.uint64)            # decreasing
    assert cc.lib.ovh_sm3_batch(cc.ctx.ptr, 2, ptr(data), ptr(bad), ptr(out)) == 103
    huge = np.array([0, 10, 1 << 32], dtype=np.uint64)      # 2^32 bytes in all
    assert cc.lib.ovh_sm3_batch(cc.ctx.ptr, 2, ptr(data), ptr(huge), ptr(out)) == 103
    assert cc.lib.ovh_sm3_batch(cc.ctx.ptr, 2, ptr(data), None, ptr(out)) == 103
    assert cc.lib.ovh_sm3_batch(cc.ctx.ptr, (1 << 24) + 1, ptr(data), ptr(bad), ptr(out)) == 103
    assert (out == 0xEE).all()
    assert cc.lib.ovh_sm3_batch(cc.ctx.ptr, 0, None, None, None) == 0
    # offsets that do not start at 0 are honoured
    good = np.array([3, 40, 64], dtype=np.uint64)
    assert cc.lib.ovh_sm3_batch(cc.ctx.ptr, 2, ptr(data), ptr(good), ptr(out)) == 0
    assert out.tobytes() == sm3(data.tobytes()[3:40]) + sm3(data.tobytes()[40:64])
