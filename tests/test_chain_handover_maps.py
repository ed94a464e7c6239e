"""CPU check of the 16-byte hand-over maps of the update's chained launches (csrc/common.h DRA_EXP_WIDE_HANDOVER), transcribed
lane by lane as tests/test_index_maps.py does for the other index arithmetic:
  * conv_v2.hip conv_fwd_v2_body, WIDE_OUT: the cross-wave fold of conv1's tile re-mapped so that a lane owns four consecutive
    positions of one output row (one ds_read_b128 per wave partial, one 16-byte store per lane);
  * conv_v2.hip conv_fwd_v2_body, WIDE_IN: conv2's row staging from float4 loads.
(The weight-gradient slab stores keep their 4-byte map: their 16-byte form measured slower and was removed.)
Every map must write every element of a tile exactly once, from the source and to the address the 4-byte map uses, and every
16-byte access must be 16-byte aligned (element offsets that are multiples of 4 behind 16-byte aligned bases)."""


def mfma_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


# ---- conv1's epilogue -------------------------------------------------------------------------------------------------------
def _fold_old(p0, np_, P):
    """{plane offset: (accumulator register, LDS lane) the four wave partials are read at, bias row}"""
    out = {}
    for wave in range(4):
        for q in range(4):
            r = wave * 4 + q
            for lane in range(64):
                li, h = lane & 31, lane >> 5
                row = mfma_row(r, h)
                if li < np_:
                    addr = row * P + p0 + li
                    assert addr not in out
                    out[addr] = (r, lane, row)
    return out


def _fold_wide(p0, np_, P):
    out, reads, stores = {}, [], []
    for wave in range(4):
        for lane in range(64):
            j, c4 = lane >> 3, lane & 7
            r = wave * 4 + (j & 3)
            slot = r * 64 + (j >> 2) * 32 + 4 * c4       # float offset inside one wave partial [16][64]
            reads.append(slot)
            bias_row = 8 * wave + (lane >> 3)
            if 4 * c4 < np_:
                off = (8 * wave + j) * P + p0 + 4 * c4
                stores.append(off)
                for k in range(4):
                    assert off + k not in out
                    out[off + k] = (r, (j >> 2) * 32 + 4 * c4 + k, bias_row)
    return out, reads, stores


def test_conv1_fold_remap_writes_what_the_dword_map_wrote():
    P, tiles = 400, 13
    for grp in range(tiles):
        p0 = grp * 32
        np_ = min(32, P - p0)
        assert np_ == (16 if grp == tiles - 1 else 32)
        old = _fold_old(p0, np_, P)
        new, reads, stores = _fold_wide(p0, np_, P)
        assert new == old, grp                                  # same source slot, same bias row, same address, once each
        assert len(old) == 32 * np_
        assert all(s % 4 == 0 for s in reads), grp              # ds_read_b128 (a wave partial is 4 KB: 16-byte aligned)
        assert all(s % 4 == 0 for s in stores), grp             # behind (sample * 32 + oc tile) * 400 floats: a multiple of 4
        assert len(stores) == (256 if np_ == 32 else 128)       # one 16-byte store per lane (half the lanes in the last tile)
    # a row's 128 bytes are written by eight lanes of ONE wave instruction
    _, _, stores = _fold_wide(0, 32, P)
    for wave in range(4):
        rows = [s // P for s in stores[64 * wave:64 * wave + 64]]
        assert rows == [8 * wave + (lane >> 3) for lane in range(64)]


# ---- conv2's staging --------------------------------------------------------------------------------------------------------
def test_conv2_row_staging_from_float4_loads():
    C, H, OH, S, KH, P = 32, 20, 9, 2, 4, 81
    WPH = (H + S - 1) // S
    RW = S * WPH
    NR = min(((31 + OH - 1) // OH) * S + KH, H)
    CS = NR * RW
    assert (NR * H) // 4 <= 64 and H % 4 == 0 and (H * H) % 4 == 0

    def col(iw):
        return (iw % S) * WPH + iw // S

    for grp in range((P + 31) // 32):
        p0 = grp * 32
        np_ = min(32, P - p0)
        oh0, oh1 = p0 // OH, (p0 + np_ - 1) // OH
        ir0, nrows = oh0 * S, (oh1 - oh0) * S + KH
        assert nrows <= NR and ir0 + nrows <= H
        for bi in (0, 5):
            old, new = {}, {}
            for wave in range(4):
                for ci in range(C // 4):
                    c = wave + 4 * ci
                    plane = (bi * C + c) * H * H
                    for lane in range(64):           # 4-byte form: 32 lanes walk a row, two rows per pass
                        rsub, iw = lane // 32, lane % 32
                        for q in range((NR + 1) // 2):
                            row = 2 * q + rsub
                            if iw < H and row < nrows:
                                old[c * CS + row * RW + col(iw)] = plane + (ir0 + row) * H + iw
                    nv = nrows * (H // 4)
                    for lane in range(64):           # 16-byte form: float4 e of the contiguous run of rows
                        e = min(lane, nv - 1)
                        row, c4 = e // (H // 4), e % (H // 4)
                        idx4 = ((bi * C + c) * H + ir0) * (H // 4) + e
                        assert idx4 * 4 == plane + ir0 * H + 4 * e           # a whole number of float4s: aligned
                        assert idx4 * 4 + 3 < (bi * C + c + 1) * H * H       # inside the channel's plane
                        if lane < nv:
                            for k in range(4):
                                dst = c * CS + row * RW + col(4 * c4 + k)
                                assert dst not in new
                                new[dst] = idx4 * 4 + k
            assert new == old, (grp, bi)
            assert len(new) == C * nrows * H
