// Owners of the per-feature host states of a pdeopt_ctx: one slot per state, created on first use.  Nothing here knows
// pdeopt_ctx, HIP or the states themselves; a state derives from Feature and frees what it owns in its destructor.
#pragma once

#include <memory>

namespace pdeopt {

struct Feature {
  virtual ~Feature() = default;
  virtual void invalidate() {}  // forget what was derived from an auxiliary field (cached multipliers and tables)
};

// declared in the order in which clear() frees them
enum FeatureSlot {
  FS_GPE_ADJOINT = 0,       // GpeAdjoint (gpe_adjoint.hip)
  FS_GPE_ROT,               // GpeRot (gpe_rot.hip)
  FS_GPE_ROT_ADJOINT,       // GpeRotAdjoint of the frozen entry point (gpe_rot_adjoint.hip)
  FS_GPE_ROT_STIR_ADJOINT,  // GpeRotAdjoint of the stirred entry point: its partial blocks differ in size
  FS_GPE_OBS,               // GpeObs (gpe_obs.hip)
  FS_SPECTRAL,              // Spectral (spectral.hip)
  FS_STRANG_FUSED,          // StrangFused (strang_fused.hip)
  FS_SENS,                  // Sens (sens.hip)
  FS_BV,                    // BvState (butler_volmer.hip)
  FS_IMPLICIT,              // Implicit (implicit.hip)
  FS_COUNT
};

class FeatureTable {
 public:
  // the state of the slot, nullptr while it is empty; T is the type the slot was filled with
  template <typename T>
  T* get(FeatureSlot s) const { return static_cast<T*>(slots_[s].get()); }
  // ... default-constructed on first use
  template <typename T>
  T& ensure(FeatureSlot s) {
    if (!slots_[s]) slots_[s] = std::make_unique<T>();
    return *static_cast<T*>(slots_[s].get());
  }
  void drop(FeatureSlot s) { slots_[s].reset(); }
  void invalidate_all() {
    for (auto& p : slots_)
      if (p) p->invalidate();
  }
  void clear() {
    for (auto& p : slots_) p.reset();
  }

 private:
  std::unique_ptr<Feature> slots_[FS_COUNT];
};

}  // namespace pdeopt
