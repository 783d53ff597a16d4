"""The shared Python plumbing between the C ABI and the reports, driven without a device: _lib.call (how an entry point
is called, with and without a caller-owned workspace), _lib.device_operand (the optional-operand check and its four
messages), _lib.host64, and main._reduced (one all-reduce for a list of blocks)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from autoreparam_amd import _lib, main, parallel

STREAM = C.c_void_p(0x5EED)


@pytest.fixture
def calls(monkeypatch):
    """A fake entry point that records its arguments, with the device context and the stream replaced by stand-ins;
    `log` holds ("device", d), ("empty", bytes) and ("fn", args) in the order they happened."""
    log = []

    @contextlib.contextmanager
    def device(d):
        log.append(("device", d))
        try:
            yield
        finally:
            log.append(("left", d))

    real_empty = torch.empty

    def empty(*size, **kw):
        log.append(("empty", size[0], kw.get("dtype"), kw.get("device")))
        return real_empty(*size, **kw)

    monkeypatch.setattr(torch.cuda, "device", device)
    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(_lib, "stream", lambda: STREAM)

    def fn(*args):
        log.append(("fn", args))
        return fn.rc
    fn.rc = 0
    fn.log = log
    return fn


def test_call_without_a_workspace_appends_the_stream_alone(calls):
    assert _lib.call("cpu", calls, 1, "two", 3.0) is None
    assert [e[0] for e in calls.log] == ["device", "fn", "left"]              # inside the device context, nothing allocated
    assert calls.log[0] == ("device", "cpu")
    assert calls.log[1][1] == (1, "two", 3.0, STREAM)


def test_call_with_a_workspace_appends_pointer_bytes_stream(calls):
    _lib.call("cpu", calls, 7, 8, workspace=96)
    assert [e[0] for e in calls.log] == ["device", "empty", "fn", "left"]
    assert calls.log[1] == ("empty", 96, torch.uint8, "cpu")                    # on the device of the call
    args = calls.log[2][1]
    assert args[:2] == (7, 8) and len(args) == 5
    pointer, need, stream = args[-3:]
    assert isinstance(pointer, C.c_void_p) and pointer.value and need == 96 and stream is STREAM


def test_call_allocates_only_for_a_positive_size(calls):
    _lib.call("cpu", calls, 7, workspace=0)
    assert [e[0] for e in calls.log] == ["device", "fn", "left"]
    pointer, need, stream = calls.log[1][1][-3:]
    assert isinstance(pointer, C.c_void_p) and not pointer.value and need == 0 and stream is STREAM      # (NULL, 0)
    assert len(calls.log[1][1]) == 4


def test_call_takes_the_size_as_the_library_returns_it(calls):
    _lib.call("cpu", calls, workspace=np.int64(32))
    assert calls.log[2][1][1] == 32 and type(calls.log[2][1][1]) is int


def test_call_raises_the_library_error_for_a_nonzero_status(calls, monkeypatch):
    class Lib(object):
        @staticmethod
        def arp_last_error():
            return b"arp_fake: refused"
    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    calls.rc = 1
    with pytest.raises(RuntimeError, match="autoreparam engine: arp_fake: refused"):
        _lib.call("cpu", calls, 1, workspace=8)
    assert calls.log[-1][0] == "left"                                           # the device context is left on the way out


class _OnGpu(torch.Tensor):
    """A host tensor that says it is on the GPU: the check reads attributes, never memory."""
    is_cuda = True


def _on_gpu(t):
    return t.as_subclass(_OnGpu)


OPERANDS = [
    (torch.int32, (4, 2, 3), "rank_normalize", "rank2", "S, C, D",
     "rank_normalize: rank2 must be a contiguous int32 [S, C, D] tensor on the GPU"),
    (torch.float32, (3,), "ess_multichain", "threshold", "D",
     "ess_multichain: threshold must be a contiguous float32 [D] tensor on the GPU"),
    (torch.float32, (3,), "gram_sums", "shift", "D", "gram_sums: shift must be a contiguous float32 [D] tensor on the GPU"),
    (torch.uint8, (7,), "psis_loo", "mask", "R", "psis_loo: mask must be a contiguous uint8 [R] tensor on the GPU"),
]


@pytest.mark.parametrize("dtype,shape,who,name,dims,message", OPERANDS, ids=[o[3] for o in OPERANDS])
def test_device_operand_messages(dtype, shape, who, name, dims, message):
    check = lambda t: _lib.device_operand(t, dtype, shape, who, name, dims)
    assert check(None) is None
    good = _on_gpu(torch.zeros(shape, dtype=dtype))
    assert check(good) is good
    other = torch.float64 if dtype != torch.float64 else torch.float32
    wide = torch.zeros(tuple(shape[:-1]) + (2 * shape[-1],), dtype=dtype)
    bad = [torch.zeros(shape, dtype=dtype),                                     # on the host
           _on_gpu(torch.zeros(shape, dtype=other)),                            # another dtype
           _on_gpu(torch.zeros(tuple(shape) + (1,), dtype=dtype)),              # another shape
           _on_gpu(wide[..., ::2]),                                             # the shape, not contiguous
           np.zeros(shape), 1.0]                                                # no tensor at all
    assert tuple(wide[..., ::2].shape) == tuple(shape) and good.is_cuda and torch.is_tensor(good)
    for t in bad:
        with pytest.raises(ValueError) as e:
            check(t)
        assert str(e.value) == message


def test_host64():
    for x in (torch.arange(6, dtype=torch.float32).reshape(2, 3), np.arange(6, dtype=np.int32).reshape(2, 3),
              [[0, 1, 2], [3, 4, 5]]):
        got = _lib.host64(x)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (2, 3)
        assert np.array_equal(got, np.arange(6.0).reshape(2, 3))
    assert _lib.host64(2.5).shape == () and np.isnan(_lib.host64(torch.tensor(float("nan"))))


def test_reduced_makes_one_all_reduce_of_the_concatenation(monkeypatch):
    sent = []

    def all_reduce_sum(value, device=None):
        sent.append((np.array(value), device))
        return torch.as_tensor(2.0 * np.asarray(value))                         # "two ranks with equal sums"

    monkeypatch.setattr(parallel, "all_reduce_sum", all_reduce_sum)
    rs = np.random.RandomState(3)
    blocks = [torch.as_tensor(rs.randn(5, 3)), rs.randn(2, 4, 3), torch.as_tensor(rs.randn(7).astype(np.float32)), 6.0,
              np.zeros((4, 0, 3)), 11]
    got = main._reduced(blocks, "dev")
    assert len(sent) == 1 and sent[0][1] == "dev"
    payload = sent[0][0]
    flat = [np.asarray(b, np.float64).ravel() for b in blocks]
    assert payload.dtype == np.float64 and payload.ndim == 1
    assert np.array_equal(payload, np.concatenate(flat))                        # every block, in order, the count where it was
    assert payload.size == 15 + 24 + 7 + 1 + 0 + 1 and payload[46] == 6.0 and payload[-1] == 11.0
    assert len(got) == len(blocks)
    for g, b in zip(got, blocks):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == np.shape(b)
        assert np.array_equal(g, 2.0 * np.asarray(b, np.float64))
    assert int(round(float(got[3]))) == 12 and int(round(float(got[5]))) == 22


def test_reduced_leaves_its_blocks_alone(monkeypatch):
    monkeypatch.setattr(parallel, "all_reduce_sum", lambda value, device=None: torch.as_tensor(np.asarray(value) + 1.0))
    a, b = torch.zeros(2, 2, dtype=torch.float64), np.zeros(3)
    got = main._reduced([a, b], None)
    assert float(a.sum()) == 0.0 and float(b.sum()) == 0.0
    assert np.array_equal(got[0], np.ones((2, 2))) and np.array_equal(got[1], np.ones(3))
