// attn_train_win.hip -- the WINDOWED (short-sequence, ragged) instance of the fused training attention (attn_train_tile.h: the kernels,
// their dataflow, the rules for rows beyond N and the budget): 128 operand columns, two 16-row tiles per wave, ONE workgroup per (window,
// head) item of 1 <= N <= 256 tokens, 4 / 7 / 8 waves by N.
#include "attn_train_tile.h"

namespace hipie {

constexpr int AW_DQ = 128;          // columns of q' / k' (4 MFMA k-steps of 32)
constexpr int AW_TR = 32;           // rows of the tile that streams through LDS per step
constexpr int AW_QT = 2;            // 16-row tiles a wave owns
constexpr int AW_MAX_N = 256;
template <int WAVES> using AtWin = AtCfg<AW_DQ, AW_QT, WAVES, AW_TR, true>;
static_assert(AtWin<8>::kFwdLds <= 64 * 1024 && AtWin<8>::kBwdKvLds <= 64 * 1024 && AtWin<8>::kBwdQLds <= 64 * 1024,
              "LDS budget: within the default dynamic limit");
static_assert(AtWin<4>::WG_ROWS == 128 && AtWin<7>::WG_ROWS == 224 && AtWin<8>::WG_ROWS == AW_MAX_N, "the wave counts of the entries below");

}  // namespace hipie

using namespace hipie;

static int at_win_check(const char* who, bool pointers, int BH, int N) {
  return at_check(who, pointers, BH, N, N <= AW_MAX_N, "BH >= 1, 1 <= N <= 256");
}

extern "C" int hipie_attn_train_win_forward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi, const void* v_lo,
                                            void* out, void* lse, int BH, int N, void* stream) {
  HIPIE_TRY(at_win_check("attn_train_win_forward", q_hi && q_lo && k_hi && k_lo && v_hi && v_lo && out && lse, BH, N));
  AtArgs a{};
  a.q_hi = q_hi, a.q_lo = q_lo, a.k_hi = k_hi, a.k_lo = k_lo, a.v_hi = v_hi, a.v_lo = v_lo, a.out = out, a.lse_out = lse;
  const auto run = N <= 128 ? at_forward<AtWin<4>> : N <= 224 ? at_forward<AtWin<7>> : at_forward<AtWin<8>>;
  run((hipStream_t)stream, (unsigned)BH, a, BH, N);
  return check_launch("attn_train_win_forward");
}

extern "C" int hipie_attn_train_win_backward(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* v_hi,
                                             const void* v_lo, const void* do_hi, const void* do_lo, const void* lse, const void* delta, void* dq,
                                             void* dk, void* dv, int BH, int N, void* stream) {
  HIPIE_TRY(at_win_check("attn_train_win_backward", q_hi && q_lo && k_hi && k_lo && v_hi && v_lo && do_hi && do_lo && lse && delta && dq && dk && dv,
                         BH, N));
  const AtArgs a{q_hi, q_lo, k_hi, k_lo, v_hi, v_lo, do_hi, do_lo, lse, delta, nullptr, nullptr, dq, dk, dv};
  const auto run = N <= 128 ? at_backward<AtWin<4>> : N <= 224 ? at_backward<AtWin<7>> : at_backward<AtWin<8>>;
  run((hipStream_t)stream, (unsigned)BH, a, BH, N);
  return check_launch("attn_train_win_backward");
}
