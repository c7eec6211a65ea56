// Stand-alone check of csrc/feature_slot.hpp with dummy features that log construction, invalidate and destruction.
// Built host-only with -fsanitize=address,undefined and run as a child process by tests/test_feature_slot_cpu.py: a double
// delete, a leak or a use after free ends the program with a sanitizer report, a wrong log with a line number and exit
// status 1.
#include <cstdio>
#include <string>

#include "feature_slot.hpp"

static std::string g_log;  // "+a" constructed, "!a" invalidated, "-a" destroyed
static int n_made = 0, n_gone = 0;

template <char TAG>
struct Dummy : pdeopt::Feature {
  int* heap = new int(TAG);  // something a leaked or twice-deleted state shows to the sanitizer
  int invalidated = 0;
  Dummy() { g_log += '+', g_log += TAG, ++n_made; }
  ~Dummy() override {
    delete heap;
    g_log += '-', g_log += TAG, ++n_gone;
  }
  void invalidate() override { g_log += '!', g_log += TAG, ++invalidated; }
};
struct Quiet : pdeopt::Feature {  // keeps the default invalidate()
  Quiet() { g_log += "+q", ++n_made; }
  ~Quiet() override { g_log += "-q", ++n_gone; }
};
using A = Dummy<'a'>;
using B = Dummy<'b'>;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::printf("FAILED line %d: %s (log \"%s\")\n", __LINE__, #cond, g_log.c_str()); \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

using namespace pdeopt;

static std::string take_log() {
  std::string s;
  s.swap(g_log);
  return s;
}

static int run() {
  FeatureTable t;
  for (int s = 0; s < FS_COUNT; ++s) CHECK(t.get<Feature>((FeatureSlot)s) == nullptr);
  // ensure constructs once and returns the same object afterwards
  A& a = t.ensure<A>(FS_SPECTRAL);
  CHECK(take_log() == "+a" && &t.ensure<A>(FS_SPECTRAL) == &a && t.get<A>(FS_SPECTRAL) == &a && g_log.empty());
  CHECK(*a.heap == 'a');
  // get is null before ensure and after drop; drop of an empty slot does nothing
  CHECK(t.get<B>(FS_SENS) == nullptr);
  t.ensure<B>(FS_SENS);
  CHECK(t.get<B>(FS_SENS) != nullptr && take_log() == "+b");
  t.drop(FS_SENS);
  CHECK(t.get<B>(FS_SENS) == nullptr && take_log() == "-b");
  t.drop(FS_SENS);
  CHECK(g_log.empty() && t.get<A>(FS_SPECTRAL) == &a);
  // two slots of one type are independent
  B& r = t.ensure<B>(FS_GPE_ROT_ADJOINT);
  B& rs = t.ensure<B>(FS_GPE_ROT_STIR_ADJOINT);
  CHECK(&r != &rs && take_log() == "+b+b");
  t.drop(FS_GPE_ROT_ADJOINT);
  CHECK(take_log() == "-b" && t.get<B>(FS_GPE_ROT_ADJOINT) == nullptr && t.get<B>(FS_GPE_ROT_STIR_ADJOINT) == &rs);
  // invalidate_all reaches exactly the live slots, in declared order; a state without an override is left alone
  t.ensure<Quiet>(FS_GPE_OBS);
  take_log();
  t.invalidate_all();
  CHECK(take_log() == "!b!a" && rs.invalidated == 1 && a.invalidated == 1);
  t.invalidate_all();
  CHECK(take_log() == "!b!a" && rs.invalidated == 2 && a.invalidated == 2);
  // clear destroys each live state once, in declared order, and leaves the table reusable
  t.ensure<B>(FS_IMPLICIT);
  t.ensure<A>(FS_GPE_ADJOINT);
  take_log();
  t.clear();
  CHECK(take_log() == "-a-b-q-a-b" && n_made == n_gone);
  for (int s = 0; s < FS_COUNT; ++s) CHECK(t.get<Feature>((FeatureSlot)s) == nullptr);
  t.clear();
  t.invalidate_all();
  CHECK(g_log.empty());
  A& again = t.ensure<A>(FS_SPECTRAL);
  CHECK(take_log() == "+a" && again.invalidated == 0 && t.get<A>(FS_SPECTRAL) == &again);
  {  // destroying a table that still holds states frees them
    FeatureTable u;
    u.ensure<A>(FS_BV);
    u.ensure<B>(FS_STRANG_FUSED);
    CHECK(take_log() == "+a+b" && n_made == n_gone + 3);
  }
  CHECK(n_made == n_gone + 1 && g_log.size() == 4);
  take_log();
  return 0;  // `t` goes with one live state: the leak check sees what it leaves
}

int main() {
  const int rc = run();
  if (rc == 0 && n_made != n_gone) {
    std::printf("FAILED: %d states made, %d destroyed\n", n_made, n_gone);
    return 1;
  }
  if (rc == 0) std::printf("feature_slot ok: %d states made, all destroyed\n", n_made);
  return rc;
}
