"""CPU model of the A-tile LDS image of wino_stream_kernel (csrc/conv_igemm.hip): 16-byte slot (row, c) of a 32-row tile sits at
row * K/4 + (c ^ (row & 15)).  Checked here, without a GPU: the DMA's source-side mapping fills every slot exactly once with the piece the
fragment reads expect, and the 16 lanes of every ds_read_b128 lane group land on 16 distinct 16-byte slots of the 256-byte bank window."""
import pytest

# the four 16-lane groups that one ds_read_b128 is serviced in (one LDS cycle each when conflict-free)
LANE_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]


def dma_image(K):
    """slot -> (row, source piece) as the kernel's DMA bookkeeping fills it: wave w, piece j, lane l feeds slot 64 (w P + j) + l."""
    cprk, P = K // 4, K // 64
    image = {}
    for wave in range(8):
        for j in range(P):
            for lane in range(64):
                slot = (wave * P + j) * 64 + lane
                r, pos = divmod(slot, cprk)
                assert slot not in image
                image[slot] = (r, pos ^ (r & 15))
    return image


def read_slot(K, lane, s, p):
    """16-byte slot that lane reads for 16-deep step s, plane p (0 = hi, 1 = lo)."""
    l32, hh = lane & 31, lane >> 5
    return l32 * (K // 4) + ((4 * s + 2 * hh + p) ^ (l32 & 15))


@pytest.mark.parametrize("K", [128, 256])      # (the kernel is written for both; K = 256 is what the library instantiates)
def test_dma_image_is_what_the_fragment_reads_expect(K):
    image = dma_image(K)
    assert sorted(image) == list(range(32 * K // 4))
    for lane in range(64):
        for s in range(K // 16):
            for p in range(2):
                # channels 16 s + 8 hh .. + 7 of row l32, plane p: piece 2 * (2 s + hh) + p of the [8 hi | 8 lo] row
                assert image[read_slot(K, lane, s, p)] == (lane & 31, 2 * (2 * s + (lane >> 5)) + p)


@pytest.mark.parametrize("K", [128, 256])
def test_fragment_reads_are_free_of_bank_conflicts(K):
    for s in range(K // 16):
        for p in range(2):
            for group in LANE_GROUPS:
                windows = {read_slot(K, lane, s, p) % 16 for lane in group}      # 16-byte slot inside the 256-byte bank window
                assert len(windows) == 16
