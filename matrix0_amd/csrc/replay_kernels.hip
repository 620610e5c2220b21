// Replaying written games on the device, one wave per game: the step before encode_positions_kernel / ssl_targets_kernel when
// the positions come from move lists (PGN, UCI lists, engine records) instead of FENs.
//   replay_games_kernel   walks a game's move patterns (san_match.h) with the search's own generator and make_move, and writes
//                         the position BEFORE every resolved move into a flat Pos array, with the move, its policy index, the
//                         legal-move count and the side to move.  Planes, masks and SSL maps of that array come from
//                         launch_encode_positions / launch_ssl_targets.
#include <hip/hip_runtime.h>
#include "tree.h"
#include "movegen_wave.h"
#include "san_match.h"

using namespace m0;

// Game g owns rows offsets[g] .. offsets[g+1] of `patterns` and of every per-ply output; it writes rows
// offsets[g] .. offsets[g] + plies[g] and leaves the others alone (the caller zeroes them).  The loop runs at most
// min(tokens, max_plies) times; every branch around a barrier is uniform in the wave.  No atomics, nothing shared between waves.
__global__ __launch_bounds__(64) void replay_games_kernel(const Pos* start, const uint32_t* patterns, const int32_t* offsets,
                                                          int n_games, int max_plies, Pos* pos_out, uint16_t* moves,
                                                          int32_t* policy_idx, int32_t* nlegal, int8_t* turn, int32_t* plies,
                                                          int32_t* status, int32_t* end_flags) {
    __shared__ Move smoves[M0_MAX_MOVES];
    __shared__ Move spseudo[M0_MAX_MOVES];
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_games) return;
    Pos p = start[g];
    const int base = offsets[g], ntok = offsets[g + 1] - base;
    const int lim = ntok < max_plies ? ntok : max_plies;
    int st = REPLAY_OK, ply = 0;
    int k = gen_legal_wave(p, smoves, spseudo, lane);
    while (ply < lim) {
        const uint32_t pat = patterns[base + ply];
        int cnt = 0;
        Move hit = 0;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            const bool ok = j < k && san_move_matches(p, smoves[j], pat);
            const unsigned long long b = __ballot(ok);
            if (b) {
                if (!cnt) hit = smoves[j0 + __ffsll((long long)b) - 1];
                cnt += __popcll(b);
            }
        }
        if (cnt != 1) { st = cnt ? REPLAY_AMBIGUOUS : REPLAY_ILLEGAL; break; }
        if (lane == 0) {
            const size_t row = (size_t)base + ply;
            pos_out[row] = p;
            moves[row] = hit;
            policy_idx[row] = move_to_index(p, hit);
            nlegal[row] = k;
            turn[row] = (int8_t)p.turn;
        }
        make_move(p, hit);
        ++ply;
        __syncthreads();                                   // every lane has read smoves before the next list is written
        k = gen_legal_wave(p, smoves, spseudo, lane);
    }
    if (st == REPLAY_OK && ntok > max_plies) st = REPLAY_TOO_LONG;
    if (lane == 0) {
        plies[g] = ply;
        status[g] = st;
        end_flags[g] = replay_end_flags(p, k);
    }
}

hipError_t launch_replay_games(const Pos* start_dev, const uint32_t* patterns_dev, const int32_t* offsets_dev, int n_games,
                               int max_plies, Pos* pos_dev, uint16_t* moves_dev, int32_t* policy_idx_dev, int32_t* nlegal_dev,
                               int8_t* turn_dev, int32_t* plies_dev, int32_t* status_dev, int32_t* end_flags_dev, hipStream_t st) {
    if (n_games <= 0) return hipSuccess;
    hipLaunchKernelGGL(replay_games_kernel, dim3(n_games), dim3(64), 0, st, start_dev, patterns_dev, offsets_dev, n_games,
                       max_plies, pos_dev, moves_dev, policy_idx_dev, nlegal_dev, turn_dev, plies_dev, status_dev, end_flags_dev);
    return hipGetLastError();
}
