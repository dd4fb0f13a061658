"""CPU model of the cross-item pipeline of wino_persist_kernel (csrc/conv_igemm.hip): one wave's stream of LDS-DMA pieces, fragment reads, counted
waits, barriers and stores in the kernel's program order, for both tile forms.  Loads, LDS-DMA and stores retire `vmcnt` in issue order, so a
wait for N leaves at most the N youngest operations outstanding.  Checked: every chunk is read from the buffer it was staged into, after the wait
that retires EVERY one of its pieces and the barrier behind it; a buffer is restaged only after the barrier that follows the lgkmcnt(0) retiring
its last reads; one operation more left outstanding, a wait without lgkmcnt(0), a missing barrier or another rotation is caught; the piece and
store counts per item are constant; the workgroups' items partition the whole range with each XCD's share contiguous.  (Only the
256 x 64 form is compiled in; the template takes both, so both are modelled.)"""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "unitspeech_amd", "csrc", "conv_igemm.hip")
FORMS = [(64, 1), (32, 2)]          # (WM, NB): 256 x 64 and 128 x 128, eight waves as 4 (M) x 2 (N)


def form_constants(wm, nb):
    mb, tm, tn = wm // 32, 4 * wm, 64 * nb
    ia, ib = tm // 8 // 8, tn // 8 // 8
    p, nst, slots = ia + ib, 4 * mb * nb, 6 * mb * nb
    return dict(P=p, NST=nst, SLOTS=slots, PSTRIDE=slots // p, TM=tm, TN=tn)


def piece_slots(k):
    """MFMA slots (0 .. SLOTS-1; phase 0 = slots below SLOTS / 2) after which a piece goes out."""
    return [j * k["PSTRIDE"] for j in range(k["P"])]


def run_schedule(k, nchunk, nitems, extra_wait=0, extra_wait_at=None, lgkm=True, barrier=True, rotation=2):
    """Replays the kernel's loop for one wave.  Returns per-item (pieces, stores).  The last five arguments are mutations the model has to
    catch: `extra_wait` operations more than the kernel's count left outstanding (at every step, or only at step (item, chunk) = `extra_wait_at`),
    the wait without its lgkmcnt(0), no barrier, chunk g + 2 staged into buffer (g + rotation) % 3.
    Every operation is known by its position in the issue order: a wait for N retires the positions below len(ops) - N.
    A buffer is 'free' (may be staged), 'reading' (this wave has fragment reads of it in flight), or 'retired' (this wave's reads are back, those
    of the other waves perhaps not: only a barrier behind every wave's lgkmcnt(0) makes it free again)."""
    P, NST, half = k["P"], k["NST"], k["SLOTS"] // 2
    slots = piece_slots(k)
    ops = []                               # issue order: ("dma", item, chunk, buf) | ("st", item)
    where = {}                             # (item, chunk) -> positions of its pieces in ops
    state = {0: "free", 1: "free", 2: "free"}
    pieces = [0] * (nitems + 1)
    stores = [0] * nitems
    issue = [0, 0]                         # item, chunk of the next pieces

    def dma(buf):
        assert state[buf] == "free", ("a buffer is restaged while reads of it may be in flight", buf, state[buf])
        where.setdefault((issue[0], issue[1]), []).append(len(ops))
        ops.append(("dma", issue[0], issue[1], buf))
        pieces[issue[0]] += 1

    def next_chunk():
        issue[1] += 1

    def start_chunk():
        if issue[1] == nchunk:
            issue[0] += 1
            issue[1] = 0

    for c in range(2):                     # prologue: chunks 0 and 1, all pieces
        start_chunk()
        for _ in range(P):
            dma(c)
        next_chunk()
    g = 0
    for it in range(nitems):
        for c in range(nchunk):
            n_wait = P + NST if (c == 1 and it != 0) else P
            if extra_wait_at is None or extra_wait_at == (it, c):
                n_wait += extra_wait
            n_retired = len(ops) - n_wait          # in-order retirement: exactly the positions below this are known to be complete
            if lgkm:
                state = {b: ("retired" if s == "reading" else s) for b, s in state.items()}
            landed = barrier                        # the other waves' pieces are known to have landed only behind a barrier
            if barrier:
                state = {b: ("free" if s == "retired" else s) for b, s in state.items()}
            cur = g % 3
            mine = where[(it, c)]
            assert len(mine) == P and max(mine) < n_retired, ("a piece of the chunk about to be read is not retired", it, c, n_wait)
            assert landed, "no barrier between the wait and the read"
            assert all(ops[i][3] == cur for i in mine), ("wrong buffer", it, c)
            buf2 = (g + rotation) % 3
            state[cur] = "reading"                  # the first fragment reads go out right behind the barrier, ahead of the first piece
            if g > 0:
                for s in slots:
                    if s < half:
                        if s == slots[0]:
                            start_chunk()
                        dma(buf2)
                if c == 0:
                    ops.extend([("st", it - 1)] * NST)
                    stores[it - 1] += NST
            else:
                start_chunk()
                for s in slots:
                    if s < half:
                        dma(buf2)
            for s in slots:
                if s >= half:
                    dma(buf2)
            next_chunk()
            g += 1
    ops.extend([("st", nitems - 1)] * NST)
    stores[nitems - 1] += NST
    return pieces, stores


@pytest.mark.parametrize("wm,nb", FORMS)
@pytest.mark.parametrize("nitems", [1, 2, 3, 7])
@pytest.mark.parametrize("nchunk", [16, 32, 64])
def test_rotation_and_wait_counts_across_items(wm, nb, nitems, nchunk):
    k = form_constants(wm, nb)
    assert k["PSTRIDE"] >= 1 and (k["P"] - 1) * k["PSTRIDE"] < k["SLOTS"] and k["P"] + k["NST"] <= 63
    pieces, stores = run_schedule(k, nchunk, nitems)
    assert pieces[:nitems] == [nchunk * k["P"]] * nitems        # constant per item ...
    assert pieces[nitems] == 2 * k["P"]                          # ... plus the two zero-filled chunks behind the last one
    assert stores == [k["NST"]] * nitems


@pytest.mark.parametrize("wm,nb", FORMS)
@pytest.mark.parametrize("at", [None, (0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 1), (2, 15)])
def test_the_counts_are_the_largest_that_are_safe(wm, nb, at):
    """One operation more left outstanding -- vmcnt(P + 1), or vmcnt(P + NST + 1) at chunk 1 of a later item -- at any kind of step, and the last
    piece of the chunk about to be read is no longer known to have landed."""
    run_schedule(form_constants(wm, nb), 16, 3, extra_wait=0, extra_wait_at=at)
    with pytest.raises(AssertionError, match="not retired"):
        run_schedule(form_constants(wm, nb), 16, 3, extra_wait=1, extra_wait_at=at)


@pytest.mark.parametrize("wm,nb", FORMS)
def test_the_model_catches_a_dropped_lgkmcnt_a_dropped_barrier_and_a_wrong_rotation(wm, nb):
    k = form_constants(wm, nb)
    with pytest.raises(AssertionError, match="restaged"):
        run_schedule(k, 16, 2, lgkm=False)
    with pytest.raises(AssertionError):
        run_schedule(k, 16, 2, barrier=False)
    for rotation in (0, 1):      # chunk g + 2 into the buffer being read, or into the one chunk g + 1 is landing in
        with pytest.raises(AssertionError):
            run_schedule(k, 16, 2, rotation=rotation)


def test_lds_fits():
    for wm, nb in FORMS:
        k = form_constants(wm, nb)
        lds = (3 * (k["TM"] + k["TN"]) * 32 + 8 * 32 * 36) * 4
        assert lds <= 160 * 1024
        if (wm, nb) == (64, 1):
            assert lds == 159744


def test_the_kernel_uses_the_modelled_counts():
    src = open(SRC).read()
    body = src[src.index("void wino_persist_kernel("):src.index("static bool wino_persist_route(")]
    assert re.search(r'if \(c == 1 && it != it_lo\) asm volatile\("s_waitcnt vmcnt\(%0\) lgkmcnt\(0\)" ::"n"\(P \+ NST\)', body)
    assert re.search(r'else asm volatile\("s_waitcnt vmcnt\(%0\) lgkmcnt\(0\)" ::"n"\(P\)', body)
    assert "constexpr int NST = 4 * MB * NB;" in body and "constexpr int PSTRIDE = SLOTS / P;" in body
    assert body.count("__builtin_amdgcn_s_barrier()") == 1 and "__syncthreads" not in body


def items_of(G, wg, total):
    """The kernel's deal: the workgroups with the same id % 8 share one contiguous part of the range; workgroup j of the gx in that group takes
    every gx-th item of it from the j-th on, so that the group is inside gx consecutive items at any time."""
    ng = min(G, 8)
    x, j = wg & 7, wg >> 3
    gx = (G - x + 7) >> 3
    return range(total * x // ng + j, total * (x + 1) // ng, gx)


@pytest.mark.parametrize("G", [1, 5, 7, 8, 9, 250, 256, 304, 1000])
@pytest.mark.parametrize("total", [1, 13, 96, 384, 1152])
def test_item_ranges_partition_the_range_with_one_contiguous_share_per_xcd(G, total):
    seen = []
    edge = 0
    for x in range(min(G, 8)):
        per_wg = [list(items_of(G, wg, total)) for wg in range(x, G, 8)]
        share = sorted(i for w in per_wg for i in w)
        assert share == list(range(edge, edge + len(share)))      # one contiguous share per XCD, the shares in XCD order, no item twice
        sizes = [len(w) for w in per_wg]
        assert max(sizes) - min(sizes) <= 1                        # dealt floor / ceil
        for s in range(max(sizes)):                                # at its s-th item the group is inside len(per_wg) consecutive items
            now = [w[s] for w in per_wg if s < len(w)]
            assert max(now) - min(now) < len(per_wg)
        edge += len(share)
        seen += share
    assert edge == total and seen == list(range(total))
