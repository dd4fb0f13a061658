"""A CPU model of store_split_pair16 (csrc/pack_f16.h).  The two-plane fp16 form keeps, per 8 channels, `8 hi | 8 lo` halves; a thread owns 4
channels and used to write its hi quad and its lo quad as two 8-byte pieces.  Now lanes 2k and 2k + 1 of a wave, which hold channel quads c and
c + 4 of one pixel / tile, exchange one quad (DPP quad_perm [1,0,3,2]: lane l reads lane l ^ 1) and each writes one whole 16-byte piece.  For the
four thread-to-channel mappings of the producers this checks that the paired stores write every byte of the image exactly once, with the value
the per-lane 8-byte stores wrote, and that both lanes of a pair always take the same bounds decision (the exchange needs its partner).
Three of the mappings run this way (wino4_input_kernel, wino_input_kernel, gn_apply_kernel); the convolution epilogue's mapping qualifies too
but keeps its 8-byte stores (the change cost the GEMM kernels more than the stores gave back)."""
import numpy as np
import pytest


def planes(idx):
    """half index of the hi quad of the channel quad at fp32-element index idx (csrc/wino.hip: store_v); lo 8 halves further"""
    return 2 * (idx & ~7) + (idx & 7)


def values(idx):
    """distinct hi / lo quads per element index: what a thread holds before the store"""
    hi = (4 * idx + np.arange(4)).astype(np.int64)
    return hi, -(hi + 1)


def store8(img, cnt, threads):
    for lane, idx in threads:
        hi, lo = values(idx)
        o = planes(idx)
        img[o:o + 4] = hi
        img[o + 8:o + 12] = lo
        cnt[o:o + 4] += 1
        cnt[o + 8:o + 12] += 1


def store16(img, cnt, threads):
    """threads: (lane, idx) of the active lanes of ONE wave instruction"""
    active = dict(threads)
    assert len(active) == len(threads)
    for lane, idx in threads:
        assert (lane ^ 1) in active, "a lane's partner must be active with it"
        odd = lane & 1
        assert ((idx >> 2) & 1) == odd, "the quad's parity is the lane's"
        hi, lo = values(idx)
        phi, plo = values(active[lane ^ 1])
        other = plo if odd else phi                 # the partner sent: even lane its lo, odd lane its hi
        first, second = (other, lo) if odd else (hi, other)
        o = planes(idx) + (4 if odd else 0)         # p + (odd ? 4 : 0) with p = this lane's hi quad
        assert o % 8 == 0                           # a 16-byte aligned piece
        img[o:o + 8] = np.concatenate([first, second])
        cnt[o:o + 8] += 1


def waves_grid_stride(per_item, C4, idx_of, grid_blocks):
    """the loop `for (i = block * 256 + thread; i < per_item; i += grid * 256)`: yields the active (lane, idx) set of every wave instruction"""
    stride = grid_blocks * 256
    for block in range(grid_blocks):
        for wave in range(4):
            base = block * 256 + wave * 64
            it = 0
            while base + it * stride < per_item:
                yield [(l, idx_of(base + l + it * stride)) for l in range(64) if base + l + it * stride < per_item]
                it += 1


def run(waves, n_halves):
    a, ca = np.zeros(n_halves, np.int64), np.zeros(n_halves, np.int64)
    b, cb = np.zeros(n_halves, np.int64), np.zeros(n_halves, np.int64)
    n = 0
    for w in waves:
        store8(a, ca, w)
        store16(b, cb, w)
        n += len(w)
    assert n > 0
    assert (ca == 1).all(), "the 8-byte stores cover the image once"
    assert (cb == 1).all(), "every byte is written exactly once"
    assert np.array_equal(a, b), "each byte carries the value the 8-byte stores wrote"


# wino4_input_kernel / wino_input_kernel: thread i = (tile, channel quad), V index = tile * C + c.  Odd tile counts, C / 4 below, equal to and
# above the wave, a grid stride that is no multiple of C / 4
@pytest.mark.parametrize("tiles,C,grid", [(85, 8, 1), (170, 256, 3), (25, 1024, 2), (9, 24, 1), (45, 520, 4)])
def test_input_transform_mapping(tiles, C, grid):
    C4 = C // 4
    per_item = tiles * C4
    run(waves_grid_stride(per_item, C4, lambda i: (i // C4) * C + (i % C4) * 4, grid), 2 * tiles * C)


# gn_apply_kernel: thread i = (pixel p, channel quad) writing row p of a tensor with leading dimension ld >= C (a multiple of 8)
@pytest.mark.parametrize("pixels,C,ld,grid", [(72 * 5, 128, 128, 2), (37, 8, 8, 1), (51, 24, 24, 1), (33, 136, 136, 3)])
def test_gn_apply_mapping(pixels, C, ld, grid):
    C4 = C // 4
    run(waves_grid_stride(pixels * C4, C4, lambda i: (i // C4) * ld + (i % C4) * 4, grid), 2 * pixels * ld)


# conv_igemm_kernel epilogue: per 32 x 32 block of a wave, lane = (row trow = lane / 8, quad tc4 = (lane % 8) * 4), four passes over rows
# trow + 8 k; rows m >= Ms and columns n >= Cout are not stored.  Ms and Cout no multiples of the block
@pytest.mark.parametrize("Ms,Cout", [(64, 64), (50, 24), (33, 72), (7, 8)])
def test_conv_epilogue_mapping(Ms, Cout):
    def waves():
        for m_base in range(0, Ms, 32):
            for ncol in range(0, Cout, 32):
                for k in range(4):
                    w = []
                    for lane in range(64):
                        m, n = m_base + (lane >> 3) + 8 * k, ncol + (lane & 7) * 4
                        if m < Ms and n < Cout:
                            w.append((lane, m * Cout + n))
                    if w:
                        yield w
    run(waves(), 2 * Ms * Cout)


def test_the_model_sees_a_broken_pairing():
    """What the launchers check before they choose the 16-byte path is what the model asserts."""
    img, cnt = np.zeros(1024, np.int64), np.zeros(1024, np.int64)
    # C = 12 in rows of 16: three quads per pixel, so lane 3 holds quad 0 of the next pixel
    with pytest.raises(AssertionError, match="parity"):
        store16(img, cnt, [(l, (l // 3) * 16 + (l % 3) * 4) for l in range(18)])
    # an odd quad count: the last lane has nobody to exchange with
    with pytest.raises(AssertionError, match="partner"):
        store16(img, cnt, [(l, l * 4) for l in range(9)])
