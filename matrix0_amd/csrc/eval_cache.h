// Device side of the per-game evaluation cache (tree.h EvalCache describes what it holds and why): key, instance and set
// address, payload layout, probe (select_kernel), victim choice and publish (expand_kernel), clear (advance_kernel).  All
// functions are whole-wave.
#pragma once
#include "tree_device.h"

constexpr int EC_WAYS = 4;
// payload words of one entry
constexpr int EC_VALUE = 0;              // network value
constexpr int EC_SIG = 1;                // legal_sig of the position's legal moves, as int bits
constexpr int EC_LOGITS = 2;             // logits of the legal moves, in generation order
static_assert(EC_LOGITS + M0_EC_MAXLEGAL == M0_EC_WORDS, "payload = value, signature, one logit per legal move");
static_assert(M0_EC_MAXLEGAL <= 64, "one legal move per lane (legal_sig)");

// The key covers what the planes and the expansion depend on: tkey (pieces, turn, cleaned castling rights, legal ep) and the
// two counters as plane_consts clips them.  Never 0 (= empty way / not cacheable).
__device__ __forceinline__ uint64_t ec_key_of(const Pos& pos) {
    const uint64_t hm = pos.halfmove < 99 ? pos.halfmove : 99, fm = pos.fullmove < 199 ? pos.fullmove : 199;
    return mix64(tkey(pos) ^ ((hm << 8 | fm) * GOLDEN64)) | 1ull;
}
// The cache instance a search of game g works on: the game's own, or in a match engine (two per game) the one of the
// network that evaluates the search.  Also the index of the instance's clock in GameDev::cache_clock.
__device__ __forceinline__ int ec_side_of(const EvalCache& ec, const GameDev* gd) { return ec.sides == 2 ? (gd->net_id & 1) : 0; }
// first way of the key's set in instance `side` of game g
__device__ __forceinline__ size_t ec_set_of(const EvalCache& ec, int g, int side, uint64_t ckey) {
    return (((size_t)g * ec.sides + side) * ec.sets + (size_t)((ckey >> 1) & (uint64_t)(ec.sets - 1))) * EC_WAYS;
}
// whole-wave: empty every instance of game g (a new game in a match engine's slot: the colours, hence the networks, swap)
__device__ __forceinline__ void ec_clear_game(const EvalCache& ec, GameDev* gd, int g, int lane) {
    const size_t n = (size_t)ec.sides * ec.sets * EC_WAYS;               // a multiple of 256 keys; the block is 16-byte aligned
    uint4* k4 = reinterpret_cast<uint4*>(ec.keys + (size_t)g * n);
    for (size_t i = lane; i < n / 2; i += 64) k4[i] = make_uint4(0, 0, 0, 0);
    if (lane == 0) { gd->cache_clock[0] = 0; gd->cache_clock[1] = 0; }
}
// where select stages the payload of sample s's hit for expand (an insert of the same pass may evict the entry)
__device__ __forceinline__ float* ec_hit_stage(const TreeDev& d, int g, int s) {
    return d.ec.hit_stage + ((size_t)g * (d.L + 1) + s) * M0_EC_WORDS;
}

// What an evaluation-cache entry stands for besides its 64-bit key: the legal-move count (low 8 bits; cacheable positions have
// at most M0_EC_MAXLEGAL = 64 moves, one per lane) and a 24-bit checksum of the legal moves in order.  A hit whose signature
// differs is a key collision and is treated as a miss: the payload's logits are stored in legal-move order, so serving them
// to another move list would expand the node with wrong priors without any other symptom.
__device__ __forceinline__ int legal_sig(const Move* mv, int n, int lane) {
    uint32_t h = lane < n ? ((uint32_t)mv[lane] + 1u) * 0x9E3779B1u + (uint32_t)lane * 0x85EBCA6Bu : 0u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 13;
    for (int o = 32; o > 0; o >>= 1) h ^= (uint32_t)__shfl_xor((int)h, o);
    return n | (int)(h & 0xFFFFFF00u);
}

// Look `ckey` up: on a key match the payload is copied to sample s's stage; a hit also needs the stored legal moves to agree
// (count and checksum: legal_sig) -- a mismatch is a key collision, served as a miss -- and refreshes the entry's stamp.
__device__ __forceinline__ bool ec_probe(const TreeDev& d, GameDev* gd, int g, int s, uint64_t ckey, const Move* legal, int nlegal,
                                         int lane) {
    bool cached = false;
    const int side = ec_side_of(d.ec, gd);
    const size_t eb = ec_set_of(d.ec, g, side, ckey);
    const uint64_t k = lane < EC_WAYS ? d.ec.keys[eb + lane] : 0ull;
    const unsigned long long hit = __ballot(lane < EC_WAYS && k == ckey);
    if (hit) {
        const int way = __builtin_ctzll(hit);
        const float* src = d.ec.payload + (eb + way) * M0_EC_WORDS;
        float* dst = ec_hit_stage(d, g, s);
        for (int i = lane; i < M0_EC_WORDS; i += 64) dst[i] = src[i];
        cached = __float_as_int(src[EC_SIG]) == legal_sig(legal, nlegal, lane);
        if (cached && lane == 0) { d.ec.stamps[eb + way] = ++gd->cache_clock[side]; }
    }
    return cached;
}

// The entry an evaluation under `ckey` goes to: the way that holds the key already, else an empty way, else the least
// recently used one (lowest way on a tie).
__device__ __forceinline__ size_t ec_choose_victim(const EvalCache& ec, const GameDev* gd, int g, uint64_t ckey, int lane) {
    const size_t eb = ec_set_of(ec, g, ec_side_of(ec, gd), ckey);
    const uint64_t k = lane < EC_WAYS ? ec.keys[eb + lane] : 0ull;
    const uint32_t st = lane < EC_WAYS ? ec.stamps[eb + lane] : 0xffffffffu;
    const unsigned long long same = __ballot(lane < EC_WAYS && k == ckey), empty = __ballot(lane < EC_WAYS && k == 0ull);
    int way;
    if (same) way = __builtin_ctzll(same);
    else if (empty) way = __builtin_ctzll(empty);
    else {
        uint32_t m = st; int w = lane;
        for (int o = EC_WAYS / 2; o > 0; o >>= 1) { const uint32_t om = __shfl_xor(m, o); const int ow = __shfl_xor(w, o); if (om < m || (om == m && ow < w)) { m = om; w = ow; } }
        way = __shfl(w, 0);
    }
    return eb + way;
}
// Rewriting entry `ce` goes: ec_invalidate, the logits into ec_payload(ce) + EC_LOGITS, ec_publish (lane 0).
__device__ __forceinline__ float* ec_payload(const EvalCache& ec, size_t ce) { return ec.payload + ce * M0_EC_WORDS; }
__device__ __forceinline__ void ec_invalidate(const EvalCache& ec, size_t ce, int lane) {
    if (lane == 0) ec.keys[ce] = 0ull;
}
__device__ __forceinline__ void ec_publish(const EvalCache& ec, GameDev* gd, size_t ce, uint64_t ckey, float v, int sig) {
    float* cw = ec_payload(ec, ce);
    cw[EC_VALUE] = v; cw[EC_SIG] = __int_as_float(sig);
    __threadfence_block();
    ec.keys[ce] = ckey; ec.stamps[ce] = ++gd->cache_clock[ec_side_of(ec, gd)];
}
