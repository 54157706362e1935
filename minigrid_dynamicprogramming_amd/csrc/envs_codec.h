// envs_codec.h -- between Grid.encode() layout and the env handle's device planes, stated once.
//
// Plain C++17 (nothing from HIP, as vi_plan.h and vi_rule.h; MGDP_HD is vi_layout.h's).  Grid.encode()
// layout is x-major (B, W, H, 3); a device plane is row-major, one byte per cell, each env padded to HWp.
// Here: the one-byte cell code, what a valid cell and a valid Box content are, the one walk over a
// batch's cells, the four conversions on top of it, the agent check, and the layout of a masked load's
// staging buffer, which the host packs and envs_masked_load_kernel reads.  A conversion that refuses
// returns a CodecError naming the cell; envs_host_state.h words it.  tests/test_envs_codec_cpu.py checks
// all of it on the CPU (tools/envs_codec_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "constants.h"
#include "vi_layout.h"

namespace mgdp {

// One-byte cell code.  Grid.encode() (grid.py:244-268) gives every cell (type, colour, state) with
// type <= 10, colour <= 5 and state != 0 only for doors (WorldObj.encode returns state 0,
// Door.encode :197-213 open 0 / closed 1 / locked 2), so a cell fits a byte: type*8 + colour, or
// 0x80 | state*8 + colour for a door.  One plane instead of three cuts the bytes the view windows
// pull from HBM by 3x (the window rows are read at cache-line granularity, i.e. most of each grid).
MGDP_HD inline uint32_t cell_code(int t, int c, int s) {
    return t == T_DOOR ? 0x80u | ((uint32_t)s << 3) | (uint32_t)c : ((uint32_t)t << 3) | (uint32_t)c;
}
MGDP_HD inline void cell_decode(uint32_t code, int &t, int &c, int &s) {
    const bool door = (code & 0x80u) != 0;
    t = door ? (int)T_DOOR : (int)(code >> 3);
    c = (int)(code & 7u);
    s = door ? (int)((code >> 3) & 3u) : 0;
}
constexpr uint32_t kCodeWall = (uint32_t)T_WALL * 8u + (uint32_t)C_GREY;  // padding / out-of-grid filler

// (t, c, s) is a cell Grid.encode() produces: what a byte cannot hold is none.
inline bool is_grid_cell(int t, int c, int s) {
    return t >= 0 && t <= T_AGENT && c >= 0 && c <= 5 && (t == T_DOOR ? s >= 0 && s <= D_LOCKED : s == 0);
}
// (t, c, s), t > T_EMPTY, is an object a Box can hold (Box(contains=...), world_object.py:272-294):
// any cell but the agent.
inline bool is_box_content(int t, int c, int s) { return t != T_AGENT && is_grid_cell(t, c, s); }

inline bool agent_in_grid(int x, int y, int d, int W, int H) { return x >= 0 && y >= 0 && x < W && y < H && d >= 0 && d < 4; }

struct CodecError {
    enum Kind { ok = 0, not_a_cell, not_an_object, not_on_a_box };
    Kind kind = ok;
    bool carried = false;     // the refused object is env b's carried one, else the one at cell (x, y)
    int b = 0, x = 0, y = 0;
    int t = 0, c = 0, s = 0;  // what was passed for it
    explicit operator bool() const { return kind != ok; }
};

struct BatchShape { int B, W, H, HWp; };

// The walk: every cell (x, y) of every env b the mask keeps (null = all), with the index of its triple
// in Grid.encode() layout and its index in a plane.  f returns false to stop the walk.
struct CellAt {
    int b, x, y;
    size_t enc, plane;
};
template <typename F>
inline void for_cells(const BatchShape &g, const uint8_t *mask, F &&f) {
    for (int b = 0; b < g.B; ++b) {
        if (mask && !mask[b]) continue;
        for (int x = 0; x < g.W; ++x)
            for (int y = 0; y < g.H; ++y)
                if (!f(CellAt{b, x, y, ((size_t)b * g.W * g.H + (size_t)x * g.H + y) * 3, (size_t)b * g.HWp + (size_t)y * g.W + x}))
                    return;
    }
}

// enc -> plane [B][HWp]: padding and the envs the mask drops hold kCodeWall; stops at the first bad cell.
inline CodecError encode_cells(const BatchShape &g, const uint8_t *enc, const uint8_t *mask, uint8_t *plane) {
    std::memset(plane, (int)kCodeWall, (size_t)g.B * g.HWp);
    CodecError err;
    for_cells(g, mask, [&](const CellAt &at) {
        const uint8_t *c = enc + at.enc;
        const int t = c[0], co = t == T_EMPTY ? 0 : c[1], st = t == T_EMPTY ? 0 : c[2];
        if (!is_grid_cell(t, co, st)) {
            err = CodecError{CodecError::not_a_cell, false, at.b, at.x, at.y, c[0], c[1], c[2]};
            return false;
        }
        plane[at.plane] = (uint8_t)cell_code(t, co, st);
        return true;
    });
    return err;
}

inline void decode_cells(const BatchShape &g, const uint8_t *plane, uint8_t *enc) {
    for_cells(g, nullptr, [&](const CellAt &at) {
        int t, c, s;
        cell_decode(plane[at.plane], t, c, s);
        uint8_t *o = enc + at.enc;
        o[0] = (uint8_t)t; o[1] = (uint8_t)c; o[2] = (uint8_t)s;
        return true;
    });
}

// A held object's code: type <= T_EMPTY (unseen / empty) = nothing held = 0.
inline bool content_code(int t, int c, int s, uint8_t &out) {
    if (t <= T_EMPTY) { out = 0; return true; }
    if (!is_box_content(t, c, s)) return false;
    out = (uint8_t)cell_code(t, c, s);
    return true;
}
inline void content_decode(uint8_t code, int &t, int &c, int &s) {
    if (code == 0) { t = c = s = 0; return; }
    cell_decode(code, t, c, s);
}

// contents (enc layout) -> contents plane, each object on a Box cell of the cell plane
inline CodecError encode_contents(const BatchShape &g, const uint8_t *contents, const uint8_t *cells, uint8_t *plane) {
    std::memset(plane, 0, (size_t)g.B * g.HWp);
    CodecError err;
    for_cells(g, nullptr, [&](const CellAt &at) {
        const uint8_t *c = contents + at.enc;
        uint8_t code;
        int t, col, st;
        cell_decode(cells[at.plane], t, col, st);
        if (!content_code(c[0], c[1], c[2], code)) err.kind = CodecError::not_an_object;
        else if (code != 0 && t != T_BOX) err.kind = CodecError::not_on_a_box;
        if (err) {
            err = CodecError{err.kind, false, at.b, at.x, at.y, c[0], c[1], c[2]};
            return false;
        }
        plane[at.plane] = code;
        return true;
    });
    return err;
}

inline void decode_contents(const BatchShape &g, const uint8_t *plane, uint8_t *contents) {
    for_cells(g, nullptr, [&](const CellAt &at) {
        int t, c, s;
        content_decode(plane[at.plane], t, c, s);
        uint8_t *o = contents + at.enc;
        o[0] = (uint8_t)t; o[1] = (uint8_t)c; o[2] = (uint8_t)s;
        return true;
    });
}

// The same for the carried object: triples [B][3] -> codes [B], each on a carried Box (carry [B][2])
inline CodecError encode_carried(int B, const int32_t *triples, const int32_t *carry, uint8_t *codes) {
    for (int b = 0; b < B; ++b) {
        const int32_t *c = triples + 3 * b;
        CodecError err{CodecError::ok, true, b, 0, 0, c[0], c[1], c[2]};
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || !content_code(c[0], c[1], c[2], codes[b])) err.kind = CodecError::not_an_object;
        else if (codes[b] != 0 && carry[2 * b] != T_BOX) err.kind = CodecError::not_on_a_box;
        if (err) return err;
    }
    return CodecError{};
}

inline void decode_carried(int B, const uint8_t *codes, int32_t *triples) {
    for (int b = 0; b < B; ++b) {
        int t, c, s;
        content_decode(codes[b], t, c, s);
        triples[3 * b] = t; triples[3 * b + 1] = c; triples[3 * b + 2] = s;
    }
}

// A masked load's staging buffer: [mask B][see B][pad to 16][cells B*HWp][agent B*4 i32][carry B*2 i32]
// [max B i32].  The sections of a buffer st (uint8_t or const uint8_t), for the host that packs it and the
// kernel that reads it; the kernel reads an env's cells as uint4: the cells' offset and HWp are multiples of 16.
struct StageLayout {
    int B, HWp;
    template <typename Byte>
    using I32 = std::conditional_t<std::is_const<Byte>::value, const int32_t, int32_t>;

    MGDP_HD int mask(int b) const { return b; }      // env b's bytes: st[mask(b)], st[see(b)]
    MGDP_HD int see(int b) const { return B + b; }
    MGDP_HD size_t cells_off() const { return (size_t)((2 * B + 15) / 16 * 16); }
    template <typename Byte>
    MGDP_HD Byte *cells(Byte *st) const { return st + cells_off(); }
    template <typename Byte>
    MGDP_HD I32<Byte> *agent(Byte *st) const { return reinterpret_cast<I32<Byte> *>(st + cells_off() + (size_t)B * HWp); }
    template <typename Byte>
    MGDP_HD I32<Byte> *carry(Byte *st) const { return agent(st) + 4 * (size_t)B; }
    template <typename Byte>
    MGDP_HD I32<Byte> *max(Byte *st) const { return carry(st) + 2 * (size_t)B; }
    MGDP_HD size_t total() const { return cells_off() + (size_t)B * HWp + sizeof(int32_t) * 7 * (size_t)B; }
};

}  // namespace mgdp
