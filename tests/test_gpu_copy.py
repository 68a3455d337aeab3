"""mip_copy_device (mipgpu.copy_device), the streaming copy bench.py calibrates the filter's HBM
roofline against.  copy_kernel is grid-stride over 16-byte words: min(ceil(n16 / 1024), 8 * CUs)
workgroups of 256 lanes, 1024 words per workgroup and iteration -- four per lane in the main loop
while `i + 768 < n16`, then one per lane in the tail loop (tests/launch_caps.py pins these
constants to the kernel's text).  The sizes here sit on every boundary of that scheme: a partial
first lane row, each of the tail loop's one to four steps, one word into the main loop, one whole
round of the capped grid minus / plus a word, a second round that only the tail loop serves, and
2 1/3 rounds.  The destination lies between two sentinel guards."""
import pytest

import launch_caps as L
import mipgpu

pytestmark = pytest.mark.gpu

GUARD = 4096                                                 # sentinel bytes before and behind dst
FILL = 0xA5
SMALL = (1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025)  # uint4 words
ROUND = ("round-1", "round", "round+1", "round+769")         # around 1024 words for every workgroup of the cap
SIZES = SMALL + ROUND + ("multipass",)


def _words(size):
    """The size in 16-byte words: one round of the capped grid is 1024 * 8 * CUs words."""
    import torch
    cap = L.copy_cap(torch.cuda.get_device_properties(0).multi_processor_count)
    one = L.COPY_WORDS_PER_GROUP * cap
    if size == "multipass":                                  # 2 1/3 rounds and half a workgroup's words
        work = L.multipass_work(cap)
        assert L.passes(work, cap) == (2, 3)
        return L.COPY_WORDS_PER_GROUP * work + 513
    return {"round-1": one - 1, "round": one, "round+1": one + 1, "round+769": one + 769}.get(size, size)


@pytest.fixture(scope="module")
def source(gpu_available):
    """Seeded random bytes on the device for the largest size and a second copy of them: the tests
    take slices and leave them unchanged."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0xC0B1)
    data = torch.randint(0, 256, (16 * _words("multipass"),), dtype=torch.uint8, device="cuda", generator=g)
    return data, data.clone()


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_copy_between_guards(gpu_available, source, size):
    """dst == src, both guards and the source untouched, on torch's current stream and on a side
    stream."""
    import torch
    n = 16 * _words(size)
    src, pristine = source[0][:n], source[1][:n]
    assert src.data_ptr() % 16 == 0
    side = torch.cuda.Stream()
    for stream in (None, side):
        buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        dst = buf[GUARD:GUARD + n]
        assert dst.data_ptr() % 16 == 0
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())   # buf is filled on the current stream
        assert mipgpu.copy_device(src, dst, stream=stream) is dst
        torch.cuda.synchronize()
        differ = torch.nonzero(dst != src)
        assert differ.numel() == 0, (size, stream is not None, differ.numel(), int(differ[0]) // 16, n // 16)
        assert bool(torch.all(buf[:GUARD] == FILL)) and bool(torch.all(buf[GUARD + n:] == FILL))
        assert torch.equal(src, pristine)


def test_copy_refusals_write_nothing(gpu_available):
    """A byte count that is no multiple of 16, a source or destination that is not 16-byte aligned,
    tensors of different sizes: MipError, and the destination keeps its bytes."""
    import torch
    src = torch.arange(256, dtype=torch.uint8, device="cuda")
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    cases = {"count": (src[:24], buf[:24]), "count-8": (src[:8], buf[:8]), "source": (src[8:72], buf[:64]),
             "destination": (src[:64], buf[8:72]), "both": (src[8:72], buf[8:72]), "sizes": (src[:64], buf[:80])}
    for name, (s, d) in cases.items():
        with pytest.raises(mipgpu.MipError):
            mipgpu.copy_device(s, d)
        torch.cuda.synchronize()
        assert bool(torch.all(buf == FILL)), name
    mipgpu.copy_device(src[16:80], buf[32:96])               # the aligned call next to them goes through
    torch.cuda.synchronize()
    assert torch.equal(buf[32:96], src[16:80]) and bool(torch.all(buf[:32] == FILL)) and bool(torch.all(buf[96:] == FILL))
