// gc_fen.h -- the FEN codec (plain C++: gc_host_base.h and include/gymchess.h only).
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/gymchess.h"
#include "gc_host_base.h"

// ----------------------------------------------------------------------------- FEN
// Forsyth-Edwards ingest/export for the reference's state: piece
// placement rank 8 first (= board row 0, lib.rs:41-50), side to move, castling -> the four
// *_castle_is_possible flags; en passant and the half-move clock do not exist under the
// reference's rules and are ignored; the full-move number n maps to move_count = n - 1
// (chess_v2.py:291-292 counts completed full moves).  Host code, no GPU needed.
static const char* FEN_PIECES = ".KQRBNP";

extern "C" int gc_fen_to_state(const char* fen, int8_t* board, uint8_t* meta) {
    return gc_fen_to_state_rules(fen, board, meta, 0);
}

// rules 1 (FIDE): the en-passant field is parsed (it must be on the rank the side to move
// captures onto) and meta8[7] = its file + 1 (0 = "-"), the engine's FIDE convention
extern "C" int gc_fen_to_state_rules(const char* fen, int8_t* board, uint8_t* meta, int rules) {
    if (!fen || !board || !meta) return fail("null argument");
    int8_t b[64] = {0};
    const char* p = fen;
    while (*p == ' ') p++;
    int row = 0, col = 0;
    for (; *p && *p != ' '; p++) {
        char c = *p;
        if (c == '/') {
            if (col != 8 || row >= 7) return fail(std::string("FEN: bad rank at '") + fen + "'");
            row++;
            col = 0;
        } else if (c >= '1' && c <= '8') {
            col += c - '0';
            if (col > 8) return fail(std::string("FEN: rank overflow in '") + fen + "'");
        } else {
            const char* q = strchr(FEN_PIECES + 1, c >= 'a' ? c - 32 : c);
            if (!q || c == '.' || col >= 8) return fail(std::string("FEN: bad piece '") + c + "' in '" + fen + "'");
            int id = (int)(q - FEN_PIECES);
            b[row * 8 + col++] = (int8_t)(c >= 'a' ? -id : id);
        }
    }
    if (row != 7 || col != 8) return fail(std::string("FEN: placement must have 8 full ranks: '") + fen + "'");
    uint8_t m[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    while (*p == ' ') p++;
    if (*p) {
        if (*p == 'b') m[0] = 0;
        else if (*p != 'w') return fail(std::string("FEN: side to move must be w or b: '") + fen + "'");
        p++;
        while (*p == ' ') p++;
        for (; *p && *p != ' '; p++) {
            switch (*p) {
                case 'K': m[1] = 1; break;
                case 'Q': m[2] = 1; break;
                case 'k': m[3] = 1; break;
                case 'q': m[4] = 1; break;
                case '-': break;
                default: return fail(std::string("FEN: bad castling field in '") + fen + "'");
            }
        }
        // reference rules: en passant and half-move clock ignored, full-move number ->
        // move_count; FIDE: en passant -> meta8[7]
        int field = 0;
        long full = 1;
        int epf = -1;
        while (*p) {
            while (*p == ' ') p++;
            if (!*p) break;
            const char* st = p;
            while (*p && *p != ' ') p++;
            ++field;
            if (field == 1 && rules && !(p - st == 1 && *st == '-')) {
                int want = m[0] ? '6' : '3';
                if (p - st != 2 || st[0] < 'a' || st[0] > 'h' || st[1] != want)
                    return fail(std::string("FEN: bad en-passant field in '") + fen + "'");
                epf = st[0] - 'a';
            }
            if (field == 3) {
                char* end = nullptr;
                full = strtol(st, &end, 10);
                if (end != p || full < 1) return fail(std::string("FEN: bad full-move number in '") + fen + "'");
            }
        }
        long mc = full - 1;
        m[7] = rules ? (uint8_t)(epf + 1) : (uint8_t)(mc > 255 ? 255 : mc);
    }
    memcpy(board, b, 64);
    memcpy(meta, m, 8);
    return 0;
}

extern "C" int gc_state_to_fen(const int8_t* board, const uint8_t* meta, char* out, int cap) {
    return gc_state_to_fen_rules(board, meta, out, cap, 0);
}

extern "C" int gc_state_to_fen_rules(const int8_t* board, const uint8_t* meta, char* out, int cap, int rules) {
    if (!board || !meta || !out) return fail("null argument");
    if (check_boards(1, board)) return -1;
    std::string f;
    for (int r = 0; r < 8; r++) {
        int gap = 0;
        for (int c = 0; c < 8; c++) {
            int v = board[r * 8 + c];
            if (!v) { gap++; continue; }
            if (gap) { f += (char)('0' + gap); gap = 0; }
            char ch = FEN_PIECES[v < 0 ? -v : v];
            f += v < 0 ? (char)(ch + 32) : ch;
        }
        if (gap) f += (char)('0' + gap);
        if (r < 7) f += '/';
    }
    f += meta[0] ? " w " : " b ";
    std::string cs;
    if (meta[1]) cs += 'K';
    if (meta[2]) cs += 'Q';
    if (meta[3]) cs += 'k';
    if (meta[4]) cs += 'q';
    f += cs.empty() ? "-" : cs;
    if (rules) {
        f += " ";
        if (meta[7]) { f += (char)('a' + ((meta[7] - 1) & 7)); f += meta[0] ? '6' : '3'; }
        else f += "-";
        f += " 0 1";
    } else {
        f += " - 0 " + std::to_string((int)meta[7] + 1);
    }
    if ((int)f.size() + 1 > cap) return fail("FEN output buffer too small");
    memcpy(out, f.c_str(), f.size() + 1);
    return 0;
}
