// What the two critic units over TRANSITION rows share (critic.hip: the particle critics, critic_checkers.hip: the Checkers critics):
// the kinds and forms, which form a kind has at which agent count -- stated ONCE, in form_exists --, the row decoding, the form
// dispatch and the argument checks of the *_rows_f32 entries.  The networks' names in the messages come from the unit.
#pragma once
#include "actor_common.h"

namespace cm3 {
namespace critic_rows {

constexpr int kGlobal = CM3_CRITIC_GLOBAL, kCredit = CM3_CRITIC_CREDIT;
constexpr int kFormRows = CM3_CRITIC_ROWS, kFormPairs = CM3_CRITIC_PAIRS, kFormCf = CM3_CRITIC_CF;

// THE rule: global takes ROWS, and CF with one agent; credit takes PAIRS and CF, and exists with more than one agent only.  Read by the
// kernels' static_assert, by check_rows (with its message) and by form_dispatch.
constexpr bool form_exists(int kind, int form, int n) {
  return kind == kGlobal ? (form == kFormRows || (form == kFormCf && n == 1)) : (n > 1 && (form == kFormPairs || form == kFormCf));
}

static const char *variant_tail(int kind, int form) {
  static const char *const kTail[2][3] = {{",kind=global,form=rows", ",kind=global,form=pairs", ",kind=global,form=cf"},
                                          {",kind=credit,form=rows", ",kind=credit,form=pairs", ",kind=credit,form=cf"}};
  return kTail[kind][form];
}

// (b, m, n, a) of row r; m = n where the form has no m, a = -1 where the action comes from the action array
template <int N, int FORM> __device__ __forceinline__ void decode(uint32_t r, uint32_t &b, int &m, int &n, int &a) {
  a = -1;
  if constexpr (FORM == kFormCf) {
    a = (int)(r % 5u);
    r /= 5u;
  }
  if constexpr (FORM == kFormRows || N == 1) {
    b = r / (uint32_t)N;
    n = (int)(r - b * (uint32_t)N);
    m = n;
  } else {
    const uint32_t t = r / (uint32_t)N;
    n = (int)(r - t * (uint32_t)N);
    b = t / (uint32_t)N;
    m = (int)(t - b * (uint32_t)N);
  }
}

// Run-time (kind, form) -> template arguments, in the style of agent_dispatch.h: f(std::integral_constant<int, KIND>,
// std::integral_constant<int, FORM>) for the combination that equals (kind, form) among those that exist at N -- only those are
// instantiated.  (The entry point has checked form_exists: the miss is for a caller that did not.)
template <int N, typename F> static int form_dispatch(int kind, int form, const char *critic, F &&f) {
  int rc = CM3_OK;
  auto at = [&](auto k, auto fm) {
    if constexpr (form_exists(k(), fm(), N)) {
      if (kind == k() && form == fm()) {
        rc = f(k, fm);
        return true;
      }
    }
    return false;
  };
  std::integral_constant<int, kGlobal> g;
  std::integral_constant<int, kCredit> c;
  std::integral_constant<int, kFormCf> cf;
  if (at(g, std::integral_constant<int, kFormRows>{}) || at(g, cf) || at(c, std::integral_constant<int, kFormPairs>{}) || at(c, cf)) return rc;
  return fail(CM3_ERR_INVALID, "the %s of kind %d has no form %d at %d agents", critic, kind, form, N);
}

// floats of the packed weights: LAYOUT<N, KIND>::kTotal (0 for an agent count outside Ns, an unknown kind, credit at N = 1)
template <template <int, int> class LAYOUT, int... Ns> static size_t floats_for(int n, int kind) {
  bool hit;
  return agent_dispatch<Ns...>(n, hit, [&](auto k) {
    constexpr int N = k();
    if (kind == kGlobal) return (size_t)LAYOUT<N, kGlobal>::kTotal;
    if (kind == kCredit && N > 1) return (size_t)LAYOUT<(N > 1 ? N : 2), kCredit>::kTotal;
    return (size_t)0;
  });
}

// the desc checks on kind and stage, behind the unit's own on desc and n_agents
static int check_kind_stage(int kind, int stage, int n_agents, const char *q_global, const char *q_credit) {
  CM3_REQUIRE(kind == kGlobal || kind == kCredit, "kind must be CM3_CRITIC_GLOBAL (0) or CM3_CRITIC_CREDIT (1), got %d", kind);
  CM3_REQUIRE(stage == 1 || stage == 2, "stage must be 1 or 2, got %d", stage);
  CM3_REQUIRE(!(kind == kCredit && (n_agents == 1 || stage == 1)), "%s exists at stage 2 with more than one agent only (n_agents %d, stage %d)",
              q_credit, n_agents, stage);
  CM3_REQUIRE((stage == 1) == (n_agents == 1), "%s runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)", q_global,
              n_agents, stage);
  return CM3_OK;
}

// What cm3_critic_rows and cm3_critic_checkers_rows (R: the same names for the fields read here) must satisfy, in the order the checks
// fire; n_rows receives the row count.  The unit's own input checks sit at two places of that order, so the entry hands them in:
// inputs_set / inputs_aligned with their texts.
template <typename R>
static int check_rows(const R *r, const void *packed, int kind, int N, const char *q_global, const char *q_credit, bool inputs_set,
                      const char *inputs_missing, bool inputs_aligned, const char *inputs_misaligned, uint32_t &n_rows) {
  CM3_REQUIRE(form_exists(kind, r->form, N), "form %d does not exist for kind %d at %d agents: %s takes ROWS (0), and CF (2) with one agent; "
              "%s takes PAIRS (1) and CF (2)", r->form, kind, N, q_global, q_credit);
  CM3_REQUIRE(r->n_steps > 0, "n_steps must be positive");
  const int64_t per_step = (int64_t)N * (r->form == kFormRows || N == 1 ? 1 : N) * (r->form == kFormCf ? kA : 1);
  CM3_REQUIRE(r->n_steps <= (int64_t)0x7fffffff / per_step, "n_steps %lld gives more than 2^31 - 1 rows (%lld per time step)",
              (long long)r->n_steps, (long long)per_step);
  CM3_REQUIRE(inputs_set, "%s", inputs_missing);
  CM3_REQUIRE(r->form == kFormCf || r->actions, "missing input: the forms ROWS and PAIRS read actions");
  CM3_REQUIRE(r->q || r->q64 || r->td, "no output requested: set q, q64 or td");
  CM3_REQUIRE(!(r->td && r->form == kFormCf), "td is not defined for the counterfactual form");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE(inputs_aligned, "%s", inputs_misaligned);
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->q % 4 == 0 && (uintptr_t)r->q64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: q must be 4-byte aligned, q64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  n_rows = (uint32_t)(r->n_steps * per_step);
  return CM3_OK;
}

}  // namespace critic_rows
}  // namespace cm3
