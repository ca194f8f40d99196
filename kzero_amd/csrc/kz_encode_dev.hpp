// kz_encode_dev.hpp — the board encode (F0) as device code: the ONE statement of encode_input_full
// (rust/kz-core/src/mapping/mod.rs:40-63) that the stand-alone kz_encode_packed kernel and every launch with a fused
// encode share.  Device code only; included INSIDE `namespace kz { namespace {` of a .hip file, after kz_kernels.hpp
// (PackedBoards).
//
// Channel order = NCHW channel order of encode_input_full: the scalar planes first (one value per board, broadcast over
// the squares), then the bool planes (mod.rs:54-59); bool i of a board = bit i % 8 of byte i / 8 of its BitBuffer
// (bit_buffer.rs:73-75), with i = plane * hw + square.  Channels beyond the planes (the padding to a multiple of 32) are
// zero.  With symmetry ids (in.sym, kz_kernels.hpp) the bool planes are read through the board's square permutation:
// the mapped board's plane at `square` is the board's own at square_src[id][square]; the scalar planes do not move.  An id
// beyond the table reads its last row (the decode reports it).  The caller keeps its own loop shape, vector width, element type and out-of-batch policy: `board` must be < batch.
// `in` is taken BY VALUE (56 bytes that already sit in kernel-argument registers): through a reference the compiler
// schedules the layer loops of kz_att_tower_mfma differently from the hand-inlined encode, by value it emits the same code.
#pragma once

__device__ __forceinline__ float encoded_plane(const PackedBoards in, int board, int ch, int square, int hw) {
    float f = 0.0f;
    if (ch < in.n_scalar) {
        f = in.scalars[(size_t)board * in.n_scalar + ch];
    } else if (ch < in.n_scalar + in.n_bool) {
        const uint8_t *bb = in.bits + (size_t)board * in.stride;
        if (in.sym) square = in.square_src[min((int)in.sym[board], in.n_sym - 1) * hw + square];
        const unsigned bit = (unsigned)(ch - in.n_scalar) * hw + square;
        f = (float)((bb[bit >> 3] >> (bit & 7)) & 1);
    }
    return f;
}
