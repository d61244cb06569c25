"""shmemx_checksum / shmemx_verify on the GPU against the host twin
(tests/gpu_util.py::checksum64), and the checksum-of-checksums property at the
bench size."""
import numpy as np
import pytest
from gpu_util import checksum64, to_dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t", ["short", "int", "long", "float", "double", "longdouble",
                               "complexd", "complexf"])
def test_checksum_matches_host_twin(cuda, shm, oracle, t):
    import torch
    for n in (0, 1, 3, 5, 64, 1001, 65537, 1 << 20):
        a = oracle.fill(t, 1, 1000 + n, n)
        if t == "longdouble" and n:
            raw = a.view(np.uint8).reshape(-1, 16)
            raw[:, 10:] = np.arange(6, dtype=np.uint8) + 1       # junk padding is ignored
        want = checksum64(a)
        assert shm.checksum(t, to_dev(torch, a), n) == want, (t, n)
        assert shm.checksum(t, a, n) == want, (t, n, "host")         # staged
    # position-aware: swapping two elements changes it
    a = oracle.fill(t, 1, 7, 100)
    b = a.copy()
    b[[3, 70]] = b[[70, 3]]
    if a[3] != a[70]:
        assert shm.checksum(t, a, 100) != shm.checksum(t, b, 100)


def test_checksum_of_checksums_full_size(cuda, shm, oracle):
    """The fold at the bench size (32 Mi doubles) checked whole by checksum:
    GPU checksum of the GPU result == host checksum of numpy's a + b."""
    import torch
    n = 32 * 1024 * 1024
    a = oracle.fill("double", 0, 11, n)
    b = oracle.fill("double", 0, 12, n)
    acc, inp = to_dev(torch, a), to_dev(torch, b)
    shm.fold("double", "sum", acc, inp, n)
    torch.cuda.synchronize()
    assert shm.checksum("double", acc, n) == checksum64(a + b)


CK_BLOCK = 256 * 16            # bytes one checksum workgroup covers per trip
CK_CAP = 2048 * CK_BLOCK       # the grid's cap: 2048 workgroups, 8 MiB


def test_checksum_grid_edges(cuda, shm):
    """The arrival tree (16 sharded counters, the top counter, the reset by the
    last workgroup) at the grid sizes where its shape changes: 1 and 2
    workgroups, 15 / 16 / 17 (nshards stops growing, shards become uneven),
    31 / 32 / 33, 2047 / 2048 (the cap) and just past it, where the grid-stride
    loop takes a second trip (the last with an odd word count).  The calls run
    in an order that mixes the sizes, so a launch that left a counter non-zero
    would spoil the next."""
    import torch
    rng = np.random.default_rng(1617)
    sizes = [k * CK_BLOCK for k in (17, 2, 2048, 1, 33, 16)] + [CK_CAP + 16, 15 * CK_BLOCK] + \
        [k * CK_BLOCK for k in (31, 32, 2047)] + [CK_CAP + CK_BLOCK + 8]
    host = rng.random(max(sizes) // 8)
    dev = to_dev(torch, host)
    want = {b: checksum64(host[:b // 8]) for b in sizes}
    assert len(set(want.values())) == len(sizes)
    for b in sizes + sizes[::-1]:
        assert shm.checksum("double", dev, b // 8) == want[b], b
    # short with a 2-byte tail, and long double (junk in the padding bytes)
    raw = rng.integers(0, 256, CK_CAP + 32, dtype=np.uint8)
    raw_dev = torch.from_numpy(raw).cuda()
    for b in (17 * CK_BLOCK, CK_CAP + 16, 17 * CK_BLOCK):
        n = b // 2 + 1
        assert shm.checksum("short", raw_dev, n) == checksum64(raw[:2 * n].view(np.int16)), b
        n = b // 16
        assert shm.checksum("longdouble", raw_dev, n) == \
            checksum64(raw[:16 * n].view(np.longdouble)), b


def test_checksum_sees_every_position(cuda, shm):
    """One flipped bit anywhere changes the value, and the GPU still agrees
    with the host twin: the first word, either side of the boundary between
    workgroups 0 and 1, the final full word of an odd word count (lane 0's
    extra term) and the last byte of the partial word behind it.  17
    workgroups' worth of shorts plus 14 bytes (one word and a 6-byte tail;
    an array of shorts has no odd byte count).  long double: bytes 10-15 of a
    slot are padding and do not count, byte 9 does."""
    import torch
    rng = np.random.default_rng(99)
    nbytes = 17 * CK_BLOCK + 14
    a = rng.integers(0, 256, nbytes, dtype=np.uint8)
    assert (nbytes // 8) % 2 == 1 and nbytes % 8 == 6
    base = shm.checksum("short", torch.from_numpy(a).cuda(), nbytes // 2)
    assert base == checksum64(a.view(np.int16))
    seen = {base}
    for pos, bit in ((0, 0), (7, 7), (CK_BLOCK - 1, 7), (CK_BLOCK - 8, 0), (CK_BLOCK, 0),
                     (17 * CK_BLOCK, 0), (17 * CK_BLOCK + 7, 7), (17 * CK_BLOCK + 8, 3),
                     (nbytes - 1, 0), (nbytes - 1, 7)):
        b = a.copy()
        b[pos] ^= 1 << bit
        got = shm.checksum("short", torch.from_numpy(b).cuda(), nbytes // 2)
        assert got == checksum64(b.view(np.int16)), (pos, bit)
        assert got not in seen, (pos, bit)
        seen.add(got)
    n = 17 * 256
    a = rng.integers(0, 256, 16 * n, dtype=np.uint8)
    base = shm.checksum("longdouble", torch.from_numpy(a).cuda(), n)
    assert base == checksum64(a.view(np.longdouble))
    for elem in (0, 255, 256, n - 1):
        for byte in range(10, 16):
            b = a.copy()
            b[16 * elem + byte] ^= 0x40
            assert shm.checksum("longdouble", torch.from_numpy(b).cuda(), n) == base, (elem, byte)
        b = a.copy()
        b[16 * elem + 9] ^= 0x40
        got = shm.checksum("longdouble", torch.from_numpy(b).cuda(), n)
        assert got != base and got == checksum64(b.view(np.longdouble)), elem


# C alignment of the element types (float _Complex: 4, double _Complex: 8)
C_ALIGN = {"short": 2, "float": 4, "double": 8, "complexf": 4, "complexd": 8}


@pytest.mark.parametrize("t", list(C_ALIGN))
def test_checksum_unaligned_device_memory(cuda, shm, oracle, t):
    """shmemx_checksum / shmemx_verify take device memory at any address the
    element type allows, not only 16-byte aligned: a reduction's target at
    heap block + 8, a slice of an array.  Every multiple of the type's C
    alignment below 16, the same elements at each: the same value as the host
    twin's, verify true, no error left behind."""
    import torch
    sz = shm.type_size(t)
    for n in (1, 3, 1001, 65537):
        a = oracle.fill(t, 1, 4242 + n, n)
        want = checksum64(a)
        data = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        buf = torch.zeros(n * sz + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        for off in range(0, 16, C_ALIGN[t]):
            buf.fill_(0x5A)
            view = buf[off:off + n * sz]
            view.copy_(data)
            torch.cuda.synchronize()
            assert shm.checksum(t, view, n) == want, (t, n, off)
            assert shm.last_error() == 0, (t, n, off)
            assert shm.verify(t, view, n, 0, 0, 1), (t, n, off)
            assert shm.last_error() == 0, (t, n, off)
            assert bool((view == data).all()), (t, n, off, "the array changed")


def test_checksum_unaligned_host_memory(cuda, shm, oracle):
    """Host memory is staged into an aligned device workspace whatever its
    own alignment, pageable or page-locked."""
    import torch
    n = 1001
    a = oracle.fill("double", 1, 77, n)
    want = checksum64(a)
    raw = np.zeros(8 * n + 32, dtype=np.uint8)
    lead = (8 - raw.ctypes.data) % 16
    pageable = raw[lead:lead + 8 * n]
    pageable[:] = a.view(np.uint8)
    assert pageable.ctypes.data % 16 == 8
    assert shm.checksum("double", pageable, n) == want
    locked = torch.zeros(8 * n + 32, dtype=torch.uint8).pin_memory()
    lead = (8 - locked.data_ptr()) % 16
    pinned = locked[lead:lead + 8 * n]
    pinned.copy_(torch.from_numpy(a.view(np.uint8)))
    assert pinned.data_ptr() % 16 == 8
    assert shm.checksum("double", pinned, n) == want
    assert shm.verify("double", pinned, n, 0, 0, 1) and shm.last_error() == 0


def test_verify_single_pe(cuda, shm):
    import torch
    x = torch.arange(1000, dtype=torch.float64, device="cuda")
    assert shm.verify("double", x, 1000, 0, 0, 1)
