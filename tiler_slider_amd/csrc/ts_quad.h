// ts_quad.h — the descriptor of the in-place step's quad store (ts_update.hip): what one board of a two-tile kernel has to
// store into its observation, packed into one 32-bit word so that the four lanes of a quad can each take one store of it.
// TS_HD like ts_core.h and for the same reason: tests/native/quad_pack_check.cpp runs these exact functions on the host over
// every cell, value and presence.  No product code path executes them on the host.
//
// A word holds four slots of eight bits, slot k in bits 8 k .. 8 k + 7: bits 0 .. 5 the cell (< 64: S <= 8), bits 6 .. 7 a code,
// 0 = nothing to store, else 1 + the value to store (0, 1 or 2: an emptied cell, tile 1, tile 2).  A word of zero stores
// nothing.  The kernel's slots are 2 t = the cell tile t enters, 2 t + 1 = the cell it leaves.
#pragma once
#include "ts_core.h"

namespace ts {

constexpr uint32_t kQuadSlots = 4;      // slots of a word, and lanes of a quad
constexpr uint32_t kQuadMaxValue = 2;   // the code has two bits
constexpr uint32_t kQuadMaxCell = 63;

// one slot: present -> cell (<= 63) and value (<= 2); absent -> 0 whatever cell and value are
TS_HD uint32_t quad_slot(bool present, uint32_t cell, uint32_t value) { return present ? (cell | ((value + 1u) << 6)) : 0u; }
// the slot as slot k (< 4) of a word
TS_HD uint32_t quad_word(uint32_t slot, uint32_t k) { return slot << (8u * k); }
// slot k (< 4) of a word, and what it says
TS_HD uint32_t quad_slot_of(uint32_t word, uint32_t k) { return (word >> (8u * k)) & 0xffu; }
TS_HD bool quad_present(uint32_t slot) { return slot >= 64u; }
TS_HD uint32_t quad_cell(uint32_t slot) { return slot & 63u; }
TS_HD uint32_t quad_value(uint32_t slot) { return (slot >> 6) - 1u; }  // of a present slot

}  // namespace ts
