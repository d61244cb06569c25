"""The gather kernel (fold_kernels.hip gather_kernel, reached through
shmemx_gather_on_stream / shm.gather) against numpy byte copies.

One gather workgroup moves 256 lanes x 8 vectors x 16 B = 32 KiB of a segment;
consecutive runs of up to 256 workgroups (8 MiB) take the segments of a launch
in turn, and the grid is sized by the longest segment, rounded up to whole
runs.  Each segment is split into a byte head (up to the target's 16-byte
boundary, clipped to the length), a 16-byte vector body and a byte tail, or is
copied byte by byte when source and target disagree mod 16.  launch_gather
drops zero-length segments before it builds the block map.

gather_launches() lays every launch out without torch or a GPU: one source and
one target buffer per launch and the segments' (source offset, target offset,
length).  test_gather_case_lists (no GPU) checks the lists themselves; the GPU
tests fill the source with random bytes and the target with a canary, launch,
and require

  * every segment's target range to equal its source range bit for bit,
  * every other byte of the target buffer to hold the canary still,
  * the source to be unchanged.

Out of scope: the cap of 65536 workgroups per segment (the grid-stride loop's
second trip) is first reached past 2 GiB per segment; the multi-PE `big`
scenario of tests/test_gpu_ipc.py walks it.
"""
import numpy as np
import pytest

BLOCK = 256 * 8 * 16          # bytes of a segment one workgroup moves
RUN = 256 * BLOCK             # bytes of a segment one run of workgroups moves
MAX_SEG = 16                  # kMaxFoldInputs
CANARY = 0xA5
MATRIX_LENGTHS = (1, 5, 15, 16, 17, 31, 33, 255, 4096 + 5)


def _layout(specs):
    """specs: (source address mod 16, target address mod 16, length), or
    (None, None, 0) for a zero-length segment with null pointers.  Places the
    segments one after another in one source and one target buffer (both
    16-byte aligned at offset 0), at least 16 canary bytes apart."""
    segs, s_cur, d_cur = [], 16, 16
    for s_mod, d_mod, length in specs:
        if s_mod is None:
            segs.append((None, None, 0))
            continue
        s_off = s_cur + (s_mod - s_cur) % 16
        d_off = d_cur + (d_mod - d_cur) % 16
        segs.append((s_off, d_off, length))
        s_cur, d_cur = s_off + length + 16, d_off + length + 16
    return {"src_size": s_cur + 16, "dst_size": d_cur + 16, "segs": segs}


def matrix_launches():
    """All 256 pairs (source mod 16, target mod 16): launch i pairs target
    offset j with source offset (i + j) % 16; the lengths rotate through
    MATRIX_LENGTHS so that a launch mixes them."""
    out = []
    for i in range(16):
        specs = [((i + j) % 16, j, MATRIX_LENGTHS[(5 * i + j) % len(MATRIX_LENGTHS)])
                 for j in range(16)]
        out.append((f"matrix-{i}", _layout(specs)))
    return out


def count_launches():
    """nseg = 1..16 with zero-length segments first, in the middle and last
    (some with null pointers, some with real ones), the longest segment (two
    workgroups' worth, so every other segment leaves a workgroup idle) in a
    different position each time; then the no-op launches."""
    out = []
    for k in range(1, MAX_SEG + 1):
        longest = (k - 1) * 5 % k
        zeros = set()
        if k > 1:
            where = {0: [0], 1: [k // 2], 2: [k - 1]}[k % 3] if k < 8 else [0, k // 2, k - 1]
            zeros = {z for z in where if z != longest}
        specs = []
        for j in range(k):
            if j in zeros:
                specs.append((None, None, 0) if (j + k) % 2 else ((3 * j) % 16, (5 * j) % 16, 0))
            elif j == longest:
                specs.append(((7 * k) % 16, (7 * k) % 16, BLOCK + 8000 + k))
            else:
                specs.append(((j + k) % 16, (3 * j) % 16 if j % 2 else (j + k) % 16, 100 + 37 * j))
        out.append((f"nseg-{k}", _layout(specs)))
    out.append(("all-zero-length", _layout([(None, None, 0), (4, 9, 0), (None, None, 0)])))
    out.append(("nseg-0", _layout([])))
    return out


def block_edge_launches():
    """The longest segment one vector short of a workgroup's 32 KiB, exactly
    that, one vector more, and two whole workgroups plus a tail byte; beside it
    100 B, exactly half its length, and one equal to it."""
    out = []
    for L in (BLOCK - 16, BLOCK, BLOCK + 16, 2 * BLOCK + 1):
        specs = [(0, 0, L), (5, 9, 100), (0, 0, L // 2), (3, 3, L)]
        out.append((f"blocks-{L}", _layout(specs)))
    return out


def run_edge_launches():
    """255, 256 and 257 workgroups' worth in the longest segment (the last
    rounds the grid up to 512 per segment, half of them idle); with it one of
    about half its length off 16-byte alignment on both sides (same offset: the
    vector path with head and tail; different offsets: bytes) and one of
    100 B."""
    out = []
    for L, mods in ((255 * BLOCK, (9, 9)), (RUN, (3, 12)), (RUN + 16, (9, 9))):
        specs = [(0, 0, L), (mods[0], mods[1], L // 2 + 3), (11, 2, 100)]
        out.append((f"run-{L}", _layout(specs)))
    return out


def gather_launches():
    return matrix_launches() + count_launches() + block_edge_launches() + run_edge_launches()


def _blocks(launch):
    """(workgroups per segment, run length) launch_gather chooses."""
    most = max([n for _, _, n in launch["segs"]] + [0])
    bx = max(1, -(-(most // 16) // 2048))
    run = min(bx, 256)
    return -(-bx // run) * run, run


def _vector_path(s_off, d_off, length):
    head = min((16 - d_off % 16) % 16, length)
    return (s_off + head) % 16 == 0, head


def test_gather_case_lists():
    """The case lists are what the GPU tests claim: in range, disjoint, and
    covering every offset pair, both copy paths, clipped heads, every segment
    count, the compaction positions and the block and run edges."""
    names = [name for name, _ in gather_launches()]
    assert len(names) == len(set(names))
    for name, L in gather_launches():
        assert len(L["segs"]) <= MAX_SEG, name
        assert L["src_size"] + L["dst_size"] <= 25 << 20, name
        spans = []
        for s_off, d_off, n in L["segs"]:
            if s_off is None:
                assert n == 0, name
                continue
            assert 16 <= s_off and s_off + n + 16 <= L["src_size"], name
            assert 16 <= d_off and d_off + n + 16 <= L["dst_size"], name
            if n:
                spans.append((d_off, d_off + n))
        spans.sort()
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), name

    m = matrix_launches()
    assert len(m) == 16 and all(len(L["segs"]) == 16 for _, L in m)
    segs = [s for _, L in m for s in L["segs"]]
    assert {(s % 16, d % 16) for s, d, _ in segs} == {(a, b) for a in range(16) for b in range(16)}
    assert {n for _, _, n in segs} == set(MATRIX_LENGTHS)
    assert all(len({n for _, _, n in L["segs"]}) >= 8 for _, L in m)
    paths = [_vector_path(*s) + (s[2],) for s in segs]
    assert any(vec and head and n > head + 16 for vec, head, n in paths)      # head, body, tail
    assert any(not vec and n > 16 for vec, head, n in paths)                   # bytes
    assert any(head == n and head for vec, head, n in paths)                   # head clipped
    assert any(vec and head == n for vec, head, n in paths)                    # ... on the vector path
    assert all(_blocks(L) == (1, 1) for _, L in m)

    c = dict(count_launches())
    assert [len(c[f"nseg-{k}"]["segs"]) for k in range(1, 17)] == list(range(1, 17))
    first = mid = last = null = real = 0
    longest_at = set()
    for k in range(1, 17):
        lens = [n for _, _, n in c[f"nseg-{k}"]["segs"]]
        assert max(lens) > BLOCK and _blocks(c[f"nseg-{k}"]) == (2, 2)
        longest_at.add(lens.index(max(lens)))
        first += lens[0] == 0
        last += k > 1 and lens[-1] == 0
        mid += any(n == 0 for n in lens[1:-1])
        null += sum(s is None for s, _, _ in c[f"nseg-{k}"]["segs"])
        real += sum(s is not None and n == 0 for s, _, n in c[f"nseg-{k}"]["segs"])
    assert first >= 3 and mid >= 3 and last >= 3 and null >= 3 and real >= 3
    assert len(longest_at) >= 10
    assert all(n == 0 for _, _, n in c["all-zero-length"]["segs"]) and c["all-zero-length"]["segs"]
    assert c["nseg-0"]["segs"] == []

    b = block_edge_launches()
    assert [_blocks(L)[0] for _, L in b] == [1, 1, 2, 2]
    for _, L in b:
        lens = [n for _, _, n in L["segs"]]
        assert lens[1] == 100 and lens[2] * 2 in (lens[0], lens[0] - 1) and lens[3] == lens[0]
    assert [L["segs"][0][2] for _, L in b] == [BLOCK - 16, BLOCK, BLOCK + 16, 2 * BLOCK + 1]

    r = run_edge_launches()
    assert [_blocks(L) for _, L in r] == [(255, 255), (256, 256), (512, 256)]
    for _, L in r:
        (s0, d0, n0), (s1, d1, n1), (_, _, n2) = L["segs"]
        assert s0 % 16 == 0 and d0 % 16 == 0 and s1 % 16 and d1 % 16
        assert abs(n1 - n0 // 2) < 16 and n2 == 100
    assert [_vector_path(*L["segs"][1])[0] for _, L in r] == [True, False, True]


def _run(torch, shm, name, L, stream=0):
    rng = np.random.default_rng(sum(name.encode()) * 7919 + L["src_size"])
    src_h = rng.integers(0, 256, L["src_size"], dtype=np.uint8)
    src = torch.from_numpy(src_h).cuda()
    dst = torch.full((L["dst_size"],), CANARY, dtype=torch.uint8, device="cuda")
    sp, dp = src.data_ptr(), dst.data_ptr()
    assert sp % 16 == 0 and dp % 16 == 0
    srcs = [None if s is None else sp + s for s, _, _ in L["segs"]]
    dsts = [None if d is None else dp + d for _, d, _ in L["segs"]]
    shm.gather(srcs, dsts, [n for _, _, n in L["segs"]], stream=stream)
    torch.cuda.synchronize()
    assert shm.last_error() == 0, name
    got = dst.cpu().numpy()
    outside = np.ones(L["dst_size"], dtype=bool)
    for k, (s, d, n) in enumerate(L["segs"]):
        if n:
            assert np.array_equal(got[d:d + n], src_h[s:s + n]), (name, k, s % 16, d % 16, n)
            outside[d:d + n] = False
    assert bool((got[outside] == CANARY).all()), (name, "wrote outside the segments")
    assert np.array_equal(src.cpu().numpy(), src_h), (name, "source changed")


@pytest.mark.gpu
def test_gather_alignment_matrix(cuda, shm):
    """Every (source mod 16, target mod 16) pair at lengths from 1 byte to a
    few KiB: heads clipped to the length, head + body + tail, the byte path."""
    import torch
    for name, L in matrix_launches():
        _run(torch, shm, name, L)


@pytest.mark.gpu
def test_gather_segment_count_and_compaction(cuda, shm):
    """1..16 segments, zero-length ones (null pointers too) dropped from the
    front, the middle and the end, short segments sharing a two-workgroup grid
    with a long one; an all-zero-length launch and nseg = 0 do nothing."""
    import torch
    for name, L in count_launches():
        _run(torch, shm, name, L)


@pytest.mark.gpu
def test_gather_block_count_edges(cuda, shm):
    """The longest segment at one vector either side of a workgroup's 32 KiB and
    one byte past two, beside shorter and equal ones."""
    import torch
    for name, L in block_edge_launches():
        _run(torch, shm, name, L)


@pytest.mark.gpu
def test_gather_run_edges(cuda, shm):
    """255, 256 and 257 workgroups per segment: one run short, one run exactly,
    and a grid rounded up to two runs with the second mostly idle."""
    import torch
    for name, L in run_edge_launches():
        _run(torch, shm, name, L)


@pytest.mark.gpu
def test_gather_argument_checks(cuda, shm):
    """More than 16 segments, and a segment whose source and target overlap,
    are refused by the host wrapper (EINVAL) before anything is launched."""
    import torch
    src = torch.arange(4096, dtype=torch.int32, device="cuda").to(torch.uint8)
    dst = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    src_h = src.cpu().numpy().copy()
    sp, dp = src.data_ptr(), dst.data_ptr()
    with pytest.raises(shm.ShmemError) as e:
        shm.gather([sp + 16 * k for k in range(17)], [dp + 16 * k for k in range(17)], [16] * 17)
    assert e.value.code == 1 and shm.last_error() == 1
    # a good segment first, then one that copies a range onto itself shifted
    with pytest.raises(shm.ShmemError) as e:
        shm.gather([sp, dp + 1000], [dp, dp + 1050], [100, 100])
    assert e.value.code == 1 and shm.last_error() == 1
    torch.cuda.synchronize()
    assert bool((dst == CANARY).all()), "a refused launch wrote"
    assert np.array_equal(src.cpu().numpy(), src_h)
    shm.gather([sp], [dp], [100])                      # and the next good call is served
    torch.cuda.synchronize()
    assert shm.last_error() == 0 and torch.equal(dst[:100], src[:100])


@pytest.mark.gpu
def test_gather_stream_order_and_kernel_clock(cuda, shm):
    """On a caller's stream the gather runs after the kernel that produced
    its source there; with the kernel clock on, the launch is reported as
    kind "gather" with its time."""
    import torch
    n = 4 << 20
    rng = np.random.default_rng(5)
    new_h = rng.integers(0, 256, n, dtype=np.uint8)
    new = torch.from_numpy(new_h).cuda()
    src = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    parts = [(0, 5, n // 2 + 1), (n // 2 + 1, n // 2 + 6 + 16, n - n // 2 - 1)]
    shm.kernel_timing(True)
    try:
        with torch.cuda.stream(s):
            src[7:7 + n].copy_(new)                    # the producer, on s
            shm.gather([src.data_ptr() + 7 + a for a, _, _ in parts],
                       [dst.data_ptr() + b for _, b, _ in parts],
                       [k for _, _, k in parts], stream=s.cuda_stream)
        s.synchronize()
        kt, dropped = shm.kernel_times()
    finally:
        shm.kernel_timing(False)
    assert [k for k, _ in kt] == ["gather"] and dropped == 0, kt
    assert 0.0 < kt[0][1] < 5000.0, kt
    got = dst.cpu().numpy()
    outside = np.ones(n + 64, dtype=bool)
    for a, b, k in parts:
        assert np.array_equal(got[b:b + k], new_h[a:a + k]), (a, b, k)
        outside[b:b + k] = False
    assert bool((got[outside] == CANARY).all())
    shm.gather([src.data_ptr()], [dst.data_ptr() + 32], [16])
    torch.cuda.synchronize()
    assert shm.kernel_times() == ([], 0)
