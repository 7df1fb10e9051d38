// sequencer.hpp — step programs: the launch sequence of a training step, recorded once at the C ABI and replayed natively.
//
// A training step of the default loop (fruitnerf_amd/training.py::TrainingSteps) is ~30 entry-point calls on two HIP
// streams with four cross-stream dependencies; every pointer in it is stable from step to step (parameter arenas,
// persistent workspaces, the step arena of per-step buffers), and only a handful of scalars change: the learning rates
// and step counts of the optimiser groups, the sampler's anneal, the random-number counter, where the five loss values
// go.  While a program is being recorded (fnr_program_begin .. fnr_program_end on the calling thread) every recordable
// entry point hands its arguments to ONE recorder, seq::record (FNR_SEQ_RECORD), and then runs as usual;
// fnr_program_replay() calls the recorded functions in order with the per-step scalars patched in.  Same entry points, same
// arguments, same streams, same order: a replayed step is the recorded step (tests/test_gpu_sequencer.py), minus the
// interpreter (0.53 -> ~0.2 ms of host time per step: what is left is the HIP runtime's own launch cost).
//
// What the recorder keeps of an argument follows from the type of the parameter it is passed for:
//   * a pointer to a host struct of the ABI (is_host_struct below): the struct, by value; the replay passes the copy's
//     address.  A NULL one means nothing is recorded (record() returns false): the call fails its own check next.
//     seq::optional(p) instead keeps NULL as NULL;
//   * a host array, wrapped at the call site as seq::host_array<MAX>(p, n): its n elements (the pointees too where they
//     are host structs); a NULL array or element stays NULL, n outside 0..MAX records nothing;
//   * everything else — device pointers, streams, numbers, internal argument blocks — by value.
// Per-step scalars enter through one customisation point, patched(x, scalars): identity by default, overloaded for
// fnr_table_adam (lr / step of its slot), for the internal blocks that carry the random-number offset (next to their
// definitions, found by argument-dependent lookup) and for three tags that wrap a bare scalar of an extern "C"
// signature at the call site: seq::Offset{offset}, seq::Anneal{anneal}, seq::Losses{losses}.  NULL scalars: every
// patch gives the recorded value.
//
// A new recordable entry point:
//   1. its first statement is FNR_SEQ_RECORD(fnr_name, <its own arguments in order>), ahead of the argument checks;
//   2. a host array goes in as seq::host_array<MAX>(p, n), a per-step scalar in its tag (a new kind of scalar: a field of
//      fnr_step_scalars, a tag and its patched() overload here);
//   3. a host struct type the ABI did not have before joins is_host_struct.
// No counterpart in the reference (its loop is nerfstudio's Python Trainer).
#pragma once
#include <array>
#include <functional>
#include <tuple>
#include <type_traits>
#include <vector>

#include "common.hpp"

namespace fnr {
namespace seq {

typedef std::function<int(const fnr_step_scalars*)> OpFn;

struct Op {
  const char* name;   // the entry point's name (static string)
  OpFn run;
};

}  // namespace seq
}  // namespace fnr

struct fnr_program {
  std::vector<fnr::seq::Op> ops;
  bool recording = false;
  const char* poisoned = nullptr;   // the entry point that ran while recording and cannot be replayed (FNR_SEQ_UNRECORDABLE)
};

namespace fnr {
namespace seq {

extern thread_local fnr_program* g_recording;

static inline bool recording() { return g_recording != nullptr; }
void push(const char* name, OpFn fn);
void poison(const char* name);

// ---- per-step scalars: patched(x, scalars) is what a replay passes for the recorded x ---------------------------------
template <class T>
static inline const T& patched(const T& x, const fnr_step_scalars*) {
  return x;
}

// lr / step of a recorded optimiser struct come from the replay's scalars when the struct names a slot
static inline fnr_table_adam patched(fnr_table_adam a, const fnr_step_scalars* s) {
  if (s && a.slot >= 1 && a.slot <= FNR_PROGRAM_ADAM_SLOTS && s->adam[a.slot - 1].step > 0) {
    a.lr = s->adam[a.slot - 1].lr;
    a.step = s->adam[a.slot - 1].step;
  }
  return a;
}

// a bare scalar of an extern "C" signature, named for what replaces it
struct Offset { uint64_t v; };   // fnr_step_scalars.prologue_offset
struct Anneal { float v; };      // .anneal
struct Losses { float* v; };     // .losses, when the replay gives one
static inline uint64_t patched(Offset o, const fnr_step_scalars* s) { return s ? s->prologue_offset : o.v; }
static inline float patched(Anneal a, const fnr_step_scalars* s) { return s ? s->anneal : a.v; }
static inline float* patched(Losses l, const fnr_step_scalars* s) { return (s && s->losses) ? s->losses : l.v; }

// ---- what is kept of an argument: ok() = the call can be recorded, get(scalars) = what the replay passes ------------------
template <class T>
constexpr bool is_host_struct =
    std::is_same_v<T, fnr_rays> || std::is_same_v<T, fnr_grid> || std::is_same_v<T, fnr_warp> || std::is_same_v<T, fnr_prop_net> ||
    std::is_same_v<T, fnr_field_net> || std::is_same_v<T, fnr_composite_options> || std::is_same_v<T, fnr_table_adam> ||
    std::is_same_v<T, fnr_image_set> || std::is_same_v<T, fnr_camera_table>;
template <class P>
constexpr bool is_host_struct_pointer = std::is_pointer_v<P> && is_host_struct<std::remove_cv_t<std::remove_pointer_t<P>>>;

template <class T>
struct Value {
  T v;
  explicit Value(const T& x) : v(x) {}
  bool ok() const { return true; }
  decltype(auto) get(const fnr_step_scalars* sc) const { return patched(v, sc); }
};

// R: T, or const T& where the patch is the identity — lives as long as the replayed call's argument list
template <class R>
struct Address {
  R v;
  bool null;
  operator const std::remove_reference_t<R>*() const { return null ? nullptr : &v; }
};

template <class T>
struct Struct {
  T v{};
  bool null, may_be_null;
  Struct(const T* p, bool may_be_null) : null(!p), may_be_null(may_be_null) {
    if (p) v = *p;
  }
  bool ok() const { return !null || may_be_null; }
  auto get(const fnr_step_scalars* sc) const { return Address<decltype(patched(v, sc))>{patched(v, sc), null}; }
};

template <class T, int MAX>
struct HostArray {
  std::array<T, MAX> v{};
  bool null, fits;
  HostArray(const T* p, int n) : null(!p), fits(n >= 0 && n <= MAX) {
    for (int i = 0; p && fits && i < n; ++i) v[i] = p[i];
  }
  bool ok() const { return fits; }
  const T* get(const fnr_step_scalars*) const { return null ? nullptr : v.data(); }
};

template <class T, int MAX>
struct HostStructArray {
  std::array<T, MAX> v{};
  std::array<bool, MAX> has{};
  bool null, fits;
  HostStructArray(const T* const* p, int n) : null(!p), fits(n >= 0 && n <= MAX) {
    for (int i = 0; p && fits && i < n; ++i)
      if (p[i]) v[i] = *p[i], has[i] = true;
  }
  bool ok() const { return fits; }
  struct Addresses {
    std::array<T, MAX> v;
    std::array<bool, MAX> has;
    bool null;
    mutable std::array<const T*, MAX> at;
    operator const T* const*() const {
      for (int i = 0; i < MAX; ++i) at[i] = has[i] ? &v[i] : nullptr;
      return null ? nullptr : at.data();
    }
  };
  Addresses get(const fnr_step_scalars* sc) const {
    Addresses a{v, has, null, {}};
    for (int i = 0; i < MAX; ++i) a.v[i] = patched(v[i], sc);
    return a;
  }
};

// ---- what a call site wraps: nothing is copied until a recording keeps it -----------------------------------------------
// a host array of n <= MAX elements; of pointers to host structs: the structs as well
template <int MAX, class T>
struct ArrayArg {
  const T* p;
  int n;
};
template <int MAX, class T>
static inline ArrayArg<MAX, T> host_array(const T* p, int n) {
  return {p, n};
}
// a pointer to a struct that the entry point accepts as NULL
template <class T>
struct OptionalArg {
  const T* p;
};
template <class T>
static inline OptionalArg<T> optional(const T* p) {
  return {p};
}

// P: the type of the parameter the argument is passed for
template <class P, class A>
static inline auto keep(const A& a) {
  if constexpr (is_host_struct_pointer<P>)
    return Struct<std::remove_cv_t<std::remove_pointer_t<P>>>(a, false);
  else
    return Value<std::decay_t<A>>(a);
}
template <class P, class T>
static inline Struct<T> keep(const OptionalArg<T>& a) {
  return Struct<T>(a.p, true);
}
template <class P, int MAX, class T>
static inline auto keep(const ArrayArg<MAX, T>& a) {
  if constexpr (is_host_struct_pointer<T>)
    return HostStructArray<std::remove_cv_t<std::remove_pointer_t<T>>, MAX>(a.p, a.n);
  else
    return HostArray<T, MAX>(a.p, a.n);
}

// records a call of fn with these arguments into the program being recorded; false when nothing was recorded
template <class... P, class... A>
bool record(const char* name, int (*fn)(P...), const A&... args) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per parameter");
  if (!recording()) return false;
  auto kept = std::make_tuple(keep<P>(args)...);
  if (!std::apply([](const auto&... k) { return (k.ok() && ...); }, kept)) return false;
  push(name, [fn, kept](const fnr_step_scalars* sc) {
    return std::apply([&](const auto&... k) { return fn(k.get(sc)...); }, kept);
  });
  return true;
}

}  // namespace seq
}  // namespace fnr

#define FNR_SEQ_RECORD(fn, ...) ::fnr::seq::record(#fn, &fn, __VA_ARGS__)

// An entry point that enqueues device work and has no recording hook: a program recorded across it would silently skip it.
#define FNR_SEQ_UNRECORDABLE(name)                          \
  do {                                                      \
    if (::fnr::seq::recording()) ::fnr::seq::poison(name);  \
  } while (0)
