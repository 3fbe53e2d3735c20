#!/usr/bin/env python3
"""Bank-conflict check, on paper, of the LDS images of the conv mode's extended frame tile (csrc/gemm_stream.hip).

A fragment read is one ds_read_b128: lane 16 g + c fetches 16-byte chunk g of one row.  The LDS serves the instruction in four
groups of 16 lanes, one LDS cycle per group when the 16 lanes hit 16 different 16-byte slots of the 256-byte bank row (bank of
byte a = (a / 4) % 64); every further distinct address on a busy slot costs the group another cycle.

  blocked form  (WFL_CONV_ROTATE=0): fragment u, lane column c, reads row r0 + 16 u + c; image: 64-byte rows, chunk XOR xswz(row)
  rotated form  (default):           fragment u, lane column c, reads row r0 + u + 6 c; image: four planes of 223 rows x 16 bytes,
                                     chunk g of row r at (223 g + r) * 16
  issue's image (not used):          (r >> 4) * 1024 + g * 256 + ((r + g) & 15) * 16 -- conflict-free too, but not linear in the row

Prints, per form, the worst multiplicity (distinct addresses on one slot within one lane group) over every start row the kernel
can use, and checks that the rotated image is a bijection between (row, chunk) and the slots the LDS-DMA fills.  No GPU needed."""
import sys

LANE_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]
TILE_ROWS = 224          # rows of the extended tile's buffer (14 pieces of 1 KiB)
XROT_ROWS = 223          # rows per plane of the rotated image (gemm_stream.hip)
MT = 6                   # 16-frame fragments per wave


def xswz(row):
    return ((row >> 2) & 1) << 1


def blocked_offset(row, g):
    return row * 64 + ((g ^ xswz(row)) << 4)


def rotated_offset(row, g):
    return (XROT_ROWS * g + row) * 16


def issue_offset(row, g):
    return (row >> 4) * 1024 + g * 256 + ((row + g) & 15) * 16


def worst_multiplicity(offset, row_of_lane_col, starts):
    """Largest number of distinct addresses that share one 16-byte slot of the bank row, over all starts and lane groups."""
    worst = 0
    for r0 in starts:
        for grp in LANE_GROUPS:
            slots = {}
            for lane in grp:
                g, c = lane >> 4, lane & 15
                a = offset(r0 + row_of_lane_col(c), g)
                assert a % 16 == 0
                slots.setdefault((a // 16) % 16, set()).add(a)
            worst = max(worst, max(len(v) for v in slots.values()))
    return worst


def dma_source(piece, lane):
    """(row, chunk) that lane `lane` of the LDS-DMA instruction filling 1 KiB piece `piece` of the rotated image fetches
    (set_src in gemm_stream.hip); the DMA puts lane l's 16 bytes at byte 1024 piece + 16 l."""
    slot = piece * 64 + lane
    ch = (slot >= XROT_ROWS) + (slot >= 2 * XROT_ROWS) + (slot >= 3 * XROT_ROWS)
    return slot - XROT_ROWS * ch, ch


def rotated_image_is_bijection():
    seen = {}
    for piece in range(TILE_ROWS // 16):
        for lane in range(64):
            row, ch = dma_source(piece, lane)
            if row >= XROT_ROWS:                      # the four padding slots behind plane 3
                continue
            if rotated_offset(row, ch) != piece * 1024 + lane * 16 or (row, ch) in seen:
                return False
            seen[(row, ch)] = True
    return len(seen) == 4 * XROT_ROWS


def report():
    # a fragment's 16 lanes span 91 rows in the rotated form (6 * 15 + 1) and 16 in the blocked one; fragment u starts u (16 u) rows on
    rot_starts = range(0, TILE_ROWS - 91 + 1)
    res = {
        "rotated reads, rotated image": worst_multiplicity(rotated_offset, lambda c: MT * c, rot_starts),
        "rotated reads, issue's image": worst_multiplicity(issue_offset, lambda c: MT * c, rot_starts),
        "rotated reads, blocked image": worst_multiplicity(blocked_offset, lambda c: MT * c, rot_starts),
        "blocked reads, blocked image (control)": worst_multiplicity(blocked_offset, lambda c: c, range(0, TILE_ROWS - 16 + 1)),
    }
    return res


def main():
    res = report()
    for k, v in res.items():
        print(f"{k:40s} worst multiplicity {v}")
    bij = rotated_image_is_bijection()
    print(f"rotated image: LDS-DMA lanes <-> (row, chunk) is a bijection onto {4 * XROT_ROWS} slots: {bij}")
    ok = res["rotated reads, rotated image"] == 1 and res["blocked reads, blocked image (control)"] == 1 and bij
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
