"""Names of the library's tuning knobs: the hand-written mirror of csrc/knobs.h (tests/test_knobs.py pins the two together).

The header holds the meanings and the defaults; the library holds the values (gnnmp.knob / gnnmp.tune / gnnmp.tuned)."""
from __future__ import annotations

import enum


class Knob(enum.IntEnum):
    FORCE_VEC = 0
    FORCE_LOG2G = 1
    UNROLL = 2
    XCD_REMAP = 3
    LONG_ROW = 4
    BLOCK_WAVES = 5
    DENSE_GENERIC = 6
    DENSE_PREFETCH = 7
    GAT_FAST_EXP = 8          # reserved (retired)
    GRADW_SLABS = 9
    GRADW_RP = 10
    GRADW_MIN_ROWS = 11
    DENSE_T16_WAVES = 12
    T16_DEBUG = 13            # libraries built with -DGNNMP_EXPERIMENTS only
    FUSED_WAVES = 14
    ROW_ORDER = 15
    SOFTMAX_ROWS = 16
    DENSE_SPLIT = 17
    CHAIN = 18
    VARIANT = 19              # a bit field of Variant
    TGCN = 20
    EDGE_DOT_GRAD = 21
    HETERO = 22
    CHUNK_SLOTS = 23


class Variant(enum.IntFlag):
    """the bits of Knob.VARIANT"""
    CHAIN_WAVES_MASK = 3      # a two-bit field, of which
    CHAIN_8_WAVES = 1         # is the one value in use
    SPLIT_SERIAL_TILES = 16
    SPLIT_DIRECT_STORES = 32
    NO_WREG = 64
    TWO_KERNEL_FOLD = 128
    WREG_SMALL = 512
