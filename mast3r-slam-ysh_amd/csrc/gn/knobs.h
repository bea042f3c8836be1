// gn/knobs.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The solver knobs: the two X-macro lists (one row per knob), KnobDef, Knobs,
// knob<>() and the M3S_TEST_KNOB accessors (constants in the product build).
// Host code only; relies on nothing but kDenseTailMin (m3s_symbolic.h).

// Solver knobs: the measured-best defaults, overridable per process by the
// environment (read ONCE, at the first use) and at run time by m3s_set_knob
// (bench legs and tests that A/B a path in one process). Each knob is declared
// once, as a row of one of the two lists below: the values (Knobs), the
// environment read, set_knob's lookup and its plan-cache drop, and the product
// build's constants are all derived from the row.
//   X(name, environment variable or nullptr, default, shapes a plan)
// The product library carries the knobs of its own paths only; the A/B
// reference paths (column-task factor, one-workgroup tail, forced dense /
// one-workgroup solves) and the bounded-wait test hook exist in the test
// build (-DM3S_TEST_PATHS: libm3s_gn_test.so, tests/conftest.py `test_lib`),
// and in the product build a test-only knob is its default as a compile-time
// constant, so no A/B branch reaches the product.
// Knobs that shape a plan (its schedule, split lists, tail, path) are not all
// in the plan-cache key: a change drops every cached plan (set_knob), so no
// launch reads a plan built for another path (e.g. a chip-path plan, cached
// unscheduled, on the one-workgroup kernel).
#define M3S_PRODUCT_KNOBS(X)                                                                                           \
  X(plan_cache, "M3S_PLAN_CACHE", 1, false)   /* 0 = symbolic analysis every call (cold calls, bench.py) */            \
  X(dense_tail_min, "M3S_DENSE_TAIL_MIN", kDenseTailMin, true) /* smallest top clique solved dense (0: never) */       \
  X(track_persistent, "M3S_TRACK_PERSISTENT", 1, false) /* 0 = one tracker launch per iteration */                     \
  X(prologue, "M3S_PROLOGUE", 1, false)       /* 0 = host prepare (ids read back, then the uploads) */
#define M3S_TEST_KNOBS(X)                                                                                              \
  X(dense, "M3S_DENSE", 0, true)              /* 1 = dense fallback LLT (only the value 1 counts) */                   \
  X(cols, "M3S_COLS", 1, true)                /* 0 = large graphs on sparse_llt_kernel's one workgroup */              \
  X(df, "M3S_DF", 1, true)                    /* 0 = column tasks + border_kernel instead of the dataflow */           \
  X(tail_cyc, "M3S_TAIL_CYC", 1, true)        /* 0 = the dense tail on one workgroup */                                \
  X(tail_mfma, "M3S_TAIL_MFMA", 1, true)      /* 0 = the dense tail in sparse_llt_kernel */                            \
  X(border_split, "M3S_BORDER_SPLIT", 1, true) /* 0 = tail border in the one-workgroup kernel */                       \
  X(debug_drop_item, nullptr, -1, true)       /* drop one LLT dispatch item (bounded-wait test) */                     \
  X(gather_lds, nullptr, 1, false)            /* 0 = the round-2 VGPR-staged gathering kernel (bitwise reference) */   \
  X(tail_pair, "M3S_TAIL_PAIR", 1, false)     /* 0 = tail_cyc_kernel (one tile column per workgroup) */                \
  X(tail_warm, "M3S_TAIL_WARM", 1, false)     /* 0 = no warm-up of the tail's diagonal factor code */                  \
  X(gcomb, "M3S_GCOMB", 1, false)             /* 0 = col_backsub_kernel after the tail, not gcol_worker */             \
  X(gcomb_wg, "M3S_GCOMB_WG", 64, false)      /* gcol_worker workgroups, >= 1 (64 measured best at 128 / 256 KFs) */   \
  /* the workers pay off once the dense tail's chain is long enough to hide the X_k recursion: 256 KFs                 \
     (42-column tail) 0.751 -> 0.712 ms per 3-iteration call, 128 KFs (a shorter tail) 0.493 -> 0.501                  \
     (profiles/r05/solve_ab_gcomb_rotated.txt) */                                                                      \
  X(gcomb_min_nc, "M3S_GCOMB_MIN_NC", 32, false) /* smallest dense tail (block columns) that takes the workers */

#define M3S_KNOB_ID(name, env, def, shaping) K_##name,
#define M3S_KNOB_DEF(name, env, def, shaping) {K_##name, #name, env, def, shaping},
#define M3S_KNOB_DEFAULT(name, env, def, shaping) \
  case K_##name: return def;
enum KnobId : int { M3S_PRODUCT_KNOBS(M3S_KNOB_ID) M3S_TEST_KNOBS(M3S_KNOB_ID) };  // = the row's index in kKnobDefs
struct KnobDef {
  KnobId id;
  const char *name, *env;
  int def;
  bool shaping;
};
constexpr KnobDef kKnobDefs[] = {  // the knobs this build knows by name
    M3S_PRODUCT_KNOBS(M3S_KNOB_DEF)
#ifdef M3S_TEST_PATHS
    M3S_TEST_KNOBS(M3S_KNOB_DEF)
#endif
};
constexpr int kNumKnobs = (int)(sizeof(kKnobDefs) / sizeof(kKnobDefs[0]));
constexpr bool knob_rows_in_id_order() {
  for (int k = 0; k < kNumKnobs; k++)
    if (kKnobDefs[k].id != k) return false;
  return true;
}
static_assert(knob_rows_in_id_order(), "Knobs::v is indexed by KnobId: row k of kKnobDefs is knob k");
constexpr int knob_default(KnobId k) {
  switch (k) {
    M3S_PRODUCT_KNOBS(M3S_KNOB_DEFAULT)
    M3S_TEST_KNOBS(M3S_KNOB_DEFAULT)
    default: return 0;
  }
}
#undef M3S_KNOB_ID
#undef M3S_KNOB_DEF
#undef M3S_KNOB_DEFAULT

struct Knobs {
  std::atomic<int> v[kNumKnobs];
  Knobs() {
    for (int k = 0; k < kNumKnobs; k++) {
      v[k] = kKnobDefs[k].def;
      if (kKnobDefs[k].env)
        if (const char *e = std::getenv(kKnobDefs[k].env)) v[k] = std::atoi(e);
    }
  }
};
Knobs &knobs() {
  static Knobs k;  // thread-safe one-time initialisation
  return k;
}
// A knob's value: the run-time one where this build has the knob, else (a
// test-only knob in the product build) its default, a compile-time constant.
template <KnobId K>
constexpr int knob() {
  if constexpr (K < kNumKnobs)
    return knobs().v[K];
  else
    return knob_default(K);
}
#ifdef M3S_TEST_PATHS
#define M3S_TEST_KNOB inline
#else
#define M3S_TEST_KNOB constexpr
#endif
M3S_TEST_KNOB bool cols_path() { return knob<K_cols>() != 0; }
M3S_TEST_KNOB bool df_path() { return knob<K_df>() != 0; }
M3S_TEST_KNOB bool tail_cyc() { return knob<K_tail_cyc>() != 0; }
M3S_TEST_KNOB bool tail_mfma() { return knob<K_tail_mfma>() != 0; }
M3S_TEST_KNOB bool border_split() { return knob<K_border_split>() != 0; }
M3S_TEST_KNOB bool force_dense_knob() { return knob<K_dense>() == 1; }
M3S_TEST_KNOB int drop_item_knob() { return knob<K_debug_drop_item>(); }
M3S_TEST_KNOB bool gather_lds_path() { return knob<K_gather_lds>() != 0; }
M3S_TEST_KNOB bool tail_pair_path() { return knob<K_tail_pair>() != 0; }
M3S_TEST_KNOB bool tail_warm_knob() { return knob<K_tail_warm>() != 0; }
M3S_TEST_KNOB bool gcomb_knob() { return knob<K_gcomb>() != 0; }
M3S_TEST_KNOB int gcomb_wg_knob() { return std::max(1, knob<K_gcomb_wg>()); }
M3S_TEST_KNOB int gcomb_min_nc_knob() { return knob<K_gcomb_min_nc>(); }
#undef M3S_TEST_KNOB
#ifndef M3S_TEST_PATHS
static_assert(cols_path() && df_path() && !force_dense_knob() && gcomb_wg_knob() == 64,
              "product build: the test-only knobs are constants");
#endif
inline int dense_tail_min() { return knob<K_dense_tail_min>(); }
inline bool plan_cache_enabled() { return knob<K_plan_cache>() != 0; }
