// seq_record_host.cpp — seq::record (fruitnerf_amd/csrc/sequencer.hpp) on the host alone: fake entry points that store what
// they are handed, recorded and replayed through the program API of sequencer.hip.  No HIP runtime call is made.  Built and
// run by tests/test_sequencer_record_cpu.py (HIP language mode, together with sequencer.hip); exit status 0 = every check
// held, otherwise the number of checks that did not (each is printed).
#include <stdarg.h>
#include <string.h>

#include <memory>
#include <utility>

#include "camera_math.hpp"
#include "sequencer.hpp"
#include "step_randoms.hpp"

namespace fnr {
void set_error(const char*, ...) {}   // (runtime.hip's, which is not linked here)
}  // namespace fnr

using namespace fnr;

static int g_failed = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++g_failed;                                                     \
      printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                 \
  } while (0)

// ---- the fake entry points: what the last call received --------------------------------------------------------------------
static struct {
  fnr_rays rays;
  fnr_composite_options opt;
  const fnr_rays* rays_at;
  int S;
  void* stream;
} g_structs;
static int fake_structs(const fnr_rays* rays, int S, const fnr_composite_options* opt, void* stream) {
  g_structs = {*rays, *opt, rays, S, stream};
  return 7;
}

static struct {
  uint64_t offset;
  float anneal;
  float* losses;
  fnr_table_adam adam;
  bool has_optional;
  fnr_table_adam optional;
} g_scalars;
static int fake_scalars(uint64_t offset, float anneal, float* losses, const fnr_table_adam* adam, const fnr_table_adam* optional) {
  g_scalars = {offset, anneal, losses, *adam, optional != nullptr, optional ? *optional : fnr_table_adam{}};
  return 0;
}

static struct {
  unsigned long long prologue_offset;
  int S0;
  bool has_edges;
  EdgeDraw edges;
  long long n_rays;
} g_blocks;
static int fake_blocks(const CameraCall& c, PrologueArgs a, const EdgeDraw* edges) {
  g_blocks = {a.offset, a.S0, edges != nullptr, edges ? *edges : EdgeDraw{}, c.n_rays};
  return 0;
}

static struct {
  int n;
  bool has_S, has_bins, has_warps, has_adam;
  int S[4];
  const float* bins[4];
  bool warp_at[4], adam_at[4];
  fnr_warp warps[4];
  fnr_table_adam adam[4];
} g_arrays;
static int fake_arrays(int n, const int* S, const float* const* bins, const fnr_warp* const* warps,
                       const fnr_table_adam* const* adam) {
  g_arrays = {};
  g_arrays.n = n, g_arrays.has_S = S, g_arrays.has_bins = bins, g_arrays.has_warps = warps, g_arrays.has_adam = adam;
  for (int i = 0; i < n; ++i) {
    if (S) g_arrays.S[i] = S[i];
    if (bins) g_arrays.bins[i] = bins[i];
    if (warps && warps[i]) g_arrays.warp_at[i] = true, g_arrays.warps[i] = *warps[i];
    if (adam && adam[i]) g_arrays.adam_at[i] = true, g_arrays.adam[i] = *adam[i];
  }
  return 0;
}

static fnr_table_adam make_adam(int slot, float lr, int64_t step) {
  fnr_table_adam a{};
  a.slot = slot, a.lr = lr, a.step = step;
  return a;
}

static fnr_step_scalars make_scalars(float* losses) {
  fnr_step_scalars sc{};
  sc.prologue_offset = 900, sc.anneal = 0.25f, sc.losses = losses;
  sc.adam[0].lr = 0.5f, sc.adam[0].step = 40;   // slot 1
  sc.adam[1].lr = 0.75f, sc.adam[1].step = 0;   // slot 2: step 0 = keep what was recorded
  return sc;
}

struct Program {
  fnr_program* p = nullptr;
  Program() { fnr_program_create(&p); }
  ~Program() { fnr_program_destroy(p); }
};

// host structs are kept by value: the caller's are overwritten (and gone) before the replay
static void structs_survive_the_callers_scope() {
  Program prog;
  EXPECT(fnr_program_begin(prog.p) == FNR_OK);
  {
    auto rays = std::make_unique<fnr_rays>();
    auto opt = std::make_unique<fnr_composite_options>();
    rays->n_rays = 11, opt->background_stride = 3;
    EXPECT(seq::record("fake_structs", &fake_structs, rays.get(), 48, opt.get(), (void*)nullptr));
    rays->n_rays = -1, opt->background_stride = -1;
  }
  // nothing is recorded for a NULL host struct, nor outside a recording
  fnr_rays rays{};
  EXPECT(!seq::record("fake_structs", &fake_structs, &rays, 48, (const fnr_composite_options*)nullptr, (void*)nullptr));
  EXPECT(fnr_program_end(prog.p) == FNR_OK && fnr_program_size(prog.p) == 1);
  fnr_composite_options opt{};
  EXPECT(!seq::record("fake_structs", &fake_structs, &rays, 48, &opt, (void*)nullptr));
  EXPECT(strcmp(fnr_program_op_name(prog.p, 0), "fake_structs") == 0);
  g_structs = {};
  EXPECT(fnr_program_replay(prog.p, nullptr) == 7);   // (the entry point's own status comes back)
  EXPECT(g_structs.rays.n_rays == 11 && g_structs.opt.background_stride == 3 && g_structs.S == 48);
  EXPECT(g_structs.rays_at != nullptr && g_structs.rays_at != &rays);
}

// the three tags, the optimiser struct and an optional struct: patched with scalars, as recorded without
static void scalars_are_patched_per_replay() {
  Program prog;
  float recorded_losses[5], step_losses[5];
  const fnr_table_adam slot1 = make_adam(1, 0.01f, 3), slot2 = make_adam(2, 0.02f, 4);
  EXPECT(fnr_program_begin(prog.p) == FNR_OK);
  EXPECT(seq::record("fake_scalars", &fake_scalars, seq::Offset{17}, seq::Anneal{1.0f}, seq::Losses{recorded_losses}, &slot1,
                     seq::optional(&slot2)));
  EXPECT(seq::record("fake_scalars", &fake_scalars, seq::Offset{17}, seq::Anneal{1.0f}, seq::Losses{recorded_losses}, &slot1,
                     seq::optional((const fnr_table_adam*)nullptr)));
  EXPECT(fnr_program_end(prog.p) == FNR_OK && fnr_program_size(prog.p) == 2);
  // a moved program replays from its own copies
  fnr_program moved = std::move(*prog.p);
  fnr_step_scalars sc = make_scalars(step_losses);
  g_scalars = {};
  EXPECT(fnr_program_replay(&moved, &sc) == FNR_OK);   // (leaves the second call's values)
  EXPECT(g_scalars.offset == 900 && g_scalars.anneal == 0.25f && g_scalars.losses == step_losses);
  EXPECT(g_scalars.adam.lr == 0.5f && g_scalars.adam.step == 40 && !g_scalars.has_optional);
  moved.ops.pop_back();
  EXPECT(fnr_program_replay(&moved, &sc) == FNR_OK);
  EXPECT(g_scalars.has_optional && g_scalars.optional.lr == 0.02f && g_scalars.optional.step == 4);   // slot 2: step 0
  sc.losses = nullptr;   // the conditional patches: no loss buffer in the scalars, a slot out of range
  sc.adam[1].step = 8;
  EXPECT(fnr_program_replay(&moved, &sc) == FNR_OK);
  EXPECT(g_scalars.offset == 900 && g_scalars.losses == recorded_losses);
  EXPECT(g_scalars.optional.lr == 0.75f && g_scalars.optional.step == 8);
  EXPECT(fnr_program_replay(&moved, nullptr) == FNR_OK);
  EXPECT(g_scalars.offset == 17 && g_scalars.anneal == 1.0f && g_scalars.losses == recorded_losses);
  EXPECT(g_scalars.adam.lr == 0.01f && g_scalars.adam.step == 3 && g_scalars.optional.lr == 0.02f);
  const fnr_table_adam no_slot = make_adam(0, 0.03f, 5), beyond = make_adam(FNR_PROGRAM_ADAM_SLOTS + 1, 0.04f, 6);
  EXPECT(seq::patched(no_slot, &sc).lr == 0.03f && seq::patched(beyond, &sc).step == 6);
}

// the internal blocks that carry the random-number offset
static void blocks_are_patched_per_replay() {
  Program prog;
  PrologueArgs a{};
  a.offset = 5, a.S0 = 64;
  const EdgeDraw drawn{1, 6, 2, 1}, given{1, 6, 2, 0};
  EXPECT(fnr_program_begin(prog.p) == FNR_OK);
  {
    const CameraCall c = camera_call("fake_blocks", nullptr, nullptr, false, FNR_POSE_SO3XR3, nullptr, 3, 77, nullptr);
    EXPECT(seq::record(c.name, &fake_blocks, c, a, seq::optional(&drawn)));
    EXPECT(seq::record(c.name, &fake_blocks, c, a, seq::optional(&given)));
    EXPECT(seq::record(c.name, &fake_blocks, c, a, seq::optional((const EdgeDraw*)nullptr)));
  }
  EXPECT(fnr_program_end(prog.p) == FNR_OK && fnr_program_size(prog.p) == 3);
  const fnr_step_scalars sc = make_scalars(nullptr);
  for (int kept = 3; kept >= 1; --kept) {   // the last op's values are what the fake keeps
    EXPECT(fnr_program_replay(prog.p, &sc) == FNR_OK);
    EXPECT(g_blocks.prologue_offset == 900 && g_blocks.S0 == 64 && g_blocks.n_rays == 77);
    EXPECT(g_blocks.has_edges == (kept < 3));
    if (kept == 2) EXPECT(g_blocks.edges.offset == 6 && g_blocks.edges.draw == 0);     // draw off: the recorded offset
    if (kept == 1) EXPECT(g_blocks.edges.offset == 900 && g_blocks.edges.level == 2);
    EXPECT(fnr_program_replay(prog.p, nullptr) == FNR_OK);
    EXPECT(g_blocks.prologue_offset == 5 && (kept == 3 || g_blocks.edges.offset == 6));
    prog.p->ops.pop_back();
  }
}

// host arrays: copied, NULL stays NULL (array or element), the pointees of struct arrays copied and patched
static void host_arrays_are_copied() {
  Program prog;
  EXPECT(fnr_program_begin(prog.p) == FNR_OK);
  {
    const float* const bins[3] = {reinterpret_cast<const float*>(64), nullptr, reinterpret_cast<const float*>(192)};
    const int S[3] = {48, 96, 8};
    fnr_warp w0{}, w2{};
    w0.mode = 1, w2.mode = 2;
    const fnr_warp* const warps[3] = {&w0, nullptr, &w2};
    const fnr_table_adam a0 = make_adam(1, 0.01f, 3), a1 = make_adam(0, 0.02f, 4);
    const fnr_table_adam* const adam[3] = {&a0, &a1, nullptr};
    EXPECT(seq::record("fake_arrays", &fake_arrays, 3, seq::host_array<4>(S, 3), seq::host_array<4>(bins, 3),
                       seq::host_array<4>(warps, 3), seq::host_array<4>(adam, 3)));
    w0.mode = -1;
    // more elements than the array holds, or fewer than none: not recorded
    EXPECT(!seq::record("fake_arrays", &fake_arrays, 5, seq::host_array<4>(S, 5), seq::host_array<4>(bins, 3),
                        seq::host_array<4>(warps, 3), seq::host_array<4>(adam, 3)));
    EXPECT(!seq::record("fake_arrays", &fake_arrays, -1, seq::host_array<4>(S, -1), seq::host_array<4>(bins, 3),
                        seq::host_array<4>(warps, 3), seq::host_array<4>(adam, 3)));
  }
  EXPECT(seq::record("fake_arrays", &fake_arrays, 2, seq::host_array<4>((const int*)nullptr, 2),
                     seq::host_array<4>((const float* const*)nullptr, 2), seq::host_array<4>((const fnr_warp* const*)nullptr, 2),
                     seq::host_array<4>((const fnr_table_adam* const*)nullptr, 2)));
  EXPECT(fnr_program_end(prog.p) == FNR_OK && fnr_program_size(prog.p) == 2);
  const fnr_step_scalars sc = make_scalars(nullptr);
  EXPECT(fnr_program_replay(prog.p, &sc) == FNR_OK);
  EXPECT(g_arrays.n == 2 && !g_arrays.has_S && !g_arrays.has_bins && !g_arrays.has_warps && !g_arrays.has_adam);
  prog.p->ops.pop_back();
  EXPECT(fnr_program_replay(prog.p, &sc) == FNR_OK);
  EXPECT(g_arrays.n == 3 && g_arrays.has_S && g_arrays.has_bins && g_arrays.has_warps && g_arrays.has_adam);
  EXPECT(g_arrays.S[0] == 48 && g_arrays.S[1] == 96 && g_arrays.S[2] == 8);
  EXPECT(g_arrays.bins[0] == reinterpret_cast<const float*>(64) && !g_arrays.bins[1] &&
         g_arrays.bins[2] == reinterpret_cast<const float*>(192));
  EXPECT(g_arrays.warp_at[0] && !g_arrays.warp_at[1] && g_arrays.warp_at[2] && g_arrays.warps[0].mode == 1 &&
         g_arrays.warps[2].mode == 2);
  EXPECT(g_arrays.adam_at[0] && g_arrays.adam_at[1] && !g_arrays.adam_at[2]);
  EXPECT(g_arrays.adam[0].lr == 0.5f && g_arrays.adam[0].step == 40 && g_arrays.adam[1].lr == 0.02f && g_arrays.adam[1].step == 4);
  EXPECT(fnr_program_replay(prog.p, nullptr) == FNR_OK);
  EXPECT(g_arrays.adam[0].lr == 0.01f && g_arrays.adam[0].step == 3);
}

int main() {
  structs_survive_the_callers_scope();
  scalars_are_patched_per_replay();
  blocks_are_patched_per_replay();
  host_arrays_are_copied();
  printf("seq_record_host: %d failed\n", g_failed);
  return g_failed;
}
