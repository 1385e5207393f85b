// Host build of the bootstrap lane function of csrc/ble_plan.h for tests/test_leaves_host.py.  TEST TOOLING: never loaded
// by the package.  Built without contraction: the lane function writes the product and the sum as two statements, which the device
// build (-ffp-contract=on) rounds separately too.
#include "../../balloon_learning_environment_amd/csrc/ble_plan.h"

using namespace ble;

extern "C" void emul_plan_bootstrap(int total, double gamma, const float* ret, const int32_t* steps_flown, const uint8_t* leaf_status,
                                    const float* value, float* score) {
  for (int j = 0; j < total; ++j) score[j] = plan_bootstrap_lane(ret[j], steps_flown[j], leaf_status[j], value[j], gamma);
}
