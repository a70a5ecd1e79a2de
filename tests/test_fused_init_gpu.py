"""The fused route of ggml_hip_mul_mat_dev (include/ggml_hip_ext.h ggml_hip_mul_mat_init_fused; csrc/gemm_qmx.hip mx_fuse): Q4_0 on 256 x 128 tiles
quantizes src1 inside the product launch, a K quarter ahead of its own loop, and hands the image from workgroup to workgroup without waiting.

The reference is the two-step route, which the fused one never touches: ggml_hip_mul_mat_init_dev + ggml_hip_mul_mat_compute_dev.  Everything is
compared bit for bit: dst, and the bytes left in the work buffer (the 48-byte bf6 image and both scale planes; the quarter of the image region
the bf6 image leaves free holds the fused launch's masks and is not compared)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

Q4_0 = 2
_W = {}


@pytest.fixture(scope="module")
def dev():
    from ggmlsharp_amd import device
    device.init(0)
    yield device
    for w in _W.values():
        w.free()
    _W.clear()


def _weight(dev, M, K):
    if (M, K) not in _W:
        g = torch.Generator(device="cuda")
        g.manual_seed(1000 * M + K)
        rows = dev.quantize_rows(Q4_0, torch.randn((M, K), generator=g, device="cuda"))
        _W[(M, K)] = dev.Weight.from_device(Q4_0, rows, K)
    return _W[(M, K)]


def _x(N, K, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn((N, K), generator=g, device="cuda") * 2


def _used(work, K, N):
    """the bytes INIT owns: the bf6 image (48 of the region's 64 bytes per row and k-block), then the two scale planes"""
    nba, Npad = (K // 32 + 3) // 4 * 4, (N + 255) // 256 * 256
    return work[:nba * 48 * Npad], work[nba * 64 * Npad:nba * 72 * Npad]


def _two_steps(dev, W, x):
    N = x.shape[0]
    work = dev.alloc_work(Q4_0, W.K, N)
    work.fill_(0x7F)                 # (rows past N are written by neither route: the same poison on both sides)
    out = torch.empty((N, W.M), device="cuda")
    dev.mul_mat_init(W, x, work)
    dev.mul_mat_compute(W, N, out, work)
    return out, work


def _assert_same(dev, W, x, out, work, what):
    ref, ref_work = _two_steps(dev, W, x)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), what
    for got, want in zip(_used(work, W.K, x.shape[0]), _used(ref_work, W.K, x.shape[0])):
        assert torch.equal(got, want), what


def _fused(dev, W, N):
    from ggmlsharp_amd._lib import lib
    return int(lib().ggml_hip_mul_mat_init_fused(W.handle, N))


# M, K, N -> is the fused route taken?  The route wants K in four quarters of eight stages (4 k-blocks each; K = 8192, sixteen, measured behind): K = 512 (four quarters of one
# stage), K = 1024, 1536, 2048 and 3072 are whole quarters but too short -- the route declines, as measured (docs/experiments/README.md); K = 544: 17
# k-blocks pad to five stages, no quarters -- declines; M = 2048 / 512 at N = 4096: the plan gives 128 x 128 / 64 x 64 tiles, not the 256 x 128 form --
# declines.  Fused: 4096^3; N = 4000: a ragged last panel and M = 4059: a ragged last row tile; the smaller row counts behind a wider src1 are
# 256 x 128 with 8 / 4 shares of 16 / 32 rows; M = 8192: 32 shares of 4 rows; N = 4100: 33 panels of 8 workgroups over 8 XCDs, so panels straddle XCDs
# and the shares written on another XCD are quantized again; K = 4064: 127 k-blocks, the last one of the image a pad block the launch writes as zeros.
SHAPES = [(4096, 512, 4096, 0), (4096, 1024, 4096, 0), (4096, 544, 4096, 0), (4096, 512, 4000, 0), (4059, 512, 4096, 0), (2048, 512, 4096, 0),
          (512, 512, 4096, 0), (4096, 2048, 4096, 0), (4096, 3072, 4096, 0), (2048, 1536, 8192, 0), (4096, 8192, 4096, 0),
          (4096, 4096, 4096, 1), (4059, 4096, 4000, 1), (2048, 4096, 8192, 1), (1024, 4096, 16384, 1), (8192, 4096, 2048, 1), (2048, 4096, 4100, 1),
          (4096, 4064, 4096, 1)]


def _masks(work, K, N):
    """the hand-off words the fused launch leaves behind the bf6 image: [16 XCC ids][panels][4] -- word 0 the shares taken on the help path,
    words 1 .. 3 the shares published per K quarter"""
    nba, Npad, panels = (K // 32 + 3) // 4 * 4, (N + 255) // 256 * 256, (N + 127) // 128
    off = nba * 48 * Npad
    return work[off:off + 16 * panels * 16].view(torch.int32).view(16, panels, 4).to(torch.int64) & 0xFFFFFFFF


@pytest.mark.parametrize("M,K,N,fused", SHAPES)
def test_fused_route_agrees_with_init_and_compute_bit_for_bit(dev, M, K, N, fused):
    W = _weight(dev, M, K)
    assert _fused(dev, W, N) == fused
    x = _x(N, K, 7)
    work = dev.alloc_work(Q4_0, K, N)
    work.fill_(0x7F)
    out = dev.mul_mat(W, x, work=work)
    _assert_same(dev, W, x, out, work, (M, K, N))


def test_the_hand_off_is_used_not_only_the_help_path(dev):
    """4096^3: every workgroup publishes its share of every quarter, and the shares come from the neighbours far more often than from the help
    path.  (How often a workgroup runs late and helps itself is a matter of timing, so the bound is loose: under half of the 15 foreign shares
    of 512 workgroups x 3 quarters; an implementation that never trusted a bit would sit at all of them.)"""
    M = K = N = 4096
    W = _weight(dev, M, K)
    assert _fused(dev, W, N) == 1
    work = dev.alloc_work(Q4_0, K, N)
    work.fill_(0x7F)
    dev.mul_mat(W, _x(N, K, 5), work=work)
    torch.cuda.synchronize()
    m = _masks(work, K, N)
    published = m[:, :, 1:].sum(dim=0)                       # bits of different XCDs are disjoint: the sum is the OR
    assert bool((published == 0xFFFF).all()), published
    helped = int(m[:, :, 0].sum())
    print("shares taken on the help path:", helped, "of", 512 * 3 * 15)
    assert helped < 512 * 3 * 15 // 2


def test_fifty_calls_on_one_work_buffer_each_with_a_fresh_src1(dev):
    """masks and image of one call must not leak into the next: the same work buffer and dst, a new x every time, every call compared"""
    M, K, N = 4096, 4096, 4096
    W = _weight(dev, M, K)
    assert _fused(dev, W, N) == 1
    work = dev.alloc_work(Q4_0, K, N)
    work.fill_(0x7F)
    out = torch.empty((N, M), device="cuda")
    for i in range(50):
        x = _x(N, K, 100 + i)
        dev.mul_mat(W, x, out=out, work=work)
        _assert_same(dev, W, x, out, work, i)


def test_help_path_serves_a_panel_whose_producers_stay_silent(dev):
    """the producers of one column panel write nothing: its consumers find the shares missing and quantize them themselves -- the same bits"""
    from ggmlsharp_amd._lib import lib
    M, K, N = 4096, 4096, 4096
    W = _weight(dev, M, K)
    assert _fused(dev, W, N) == 1
    x = _x(N, K, 11)
    try:
        for panel in (0, 13, 31):
            lib().ggml_hip_debug_fused_init_skip_panel(panel)
            work = dev.alloc_work(Q4_0, K, N)
            work.fill_(0x7F)
            out = dev.mul_mat(W, x, work=work)
            _assert_same(dev, W, x, out, work, panel)
            m = _masks(work, K, N)
            assert int(m[:, panel, 1:].sum()) == 0           # nothing published for the panel ..
            assert int(m[:, panel, 0].sum()) == 16 * 3 * 16  # .. and each of its 16 workgroups took all 16 shares of 3 quarters itself
    finally:
        lib().ggml_hip_debug_fused_init_skip_panel(-1)


def test_two_streams_with_a_work_buffer_each_run_side_by_side(dev):
    M, K, N = 4096, 4096, 4096
    W = _weight(dev, M, K)
    xs = [_x(N, K, 21), _x(N, K, 22)]
    refs = [_two_steps(dev, W, x) for x in xs]
    works = [dev.alloc_work(Q4_0, K, N) for _ in xs]
    outs = [torch.empty((N, M), device="cuda") for _ in xs]
    for w in works:
        w.fill_(0x7F)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(4):
        for s, x, o, w in zip(streams, xs, outs, works):
            with torch.cuda.stream(s):
                dev.mul_mat(W, x, out=o, work=w)
    torch.cuda.synchronize()
    for x, o, w, (ref, ref_work) in zip(xs, outs, works, refs):
        assert torch.equal(o, ref)
        for got, want in zip(_used(w, K, N), _used(ref_work, K, N)):
            assert torch.equal(got, want)
