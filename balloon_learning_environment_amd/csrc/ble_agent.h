// ble_agent.h -- the StationSeeker controller (agents/station_seeker_agent.py:72-186 of the reference) and the per-step
// bookkeeping of its evaluation loop (eval/eval_lib.py:157-190), on the device.
//
// Seeker: one wave64 per environment.  Lane l owns the relative levels l, l + 64, ..., l + 320 (six for lanes 0-40, five for the
// rest); its loads of the (uncertainty, bearing, magnitude) triples are coalesced across the wave.  The score is the reference's
// float64 expression on the float32 features (NumPy's promotion):
//   bearing   = 0 + b * pi,  magnitude = 30 m / (1 - m)                       features.py:229-266 (un-rescale, un-squash)
//   distance  = 250 d / (1 - d)   (d = feature 7)                             station_seeker_agent.py:164-165
//   coeff     = clip((distance - 250) / 250, 0, 1),  w = 0.6 + coeff (0.45 - 0.6),  alpha_delta = exp(-distance / 35)
//   wind      = (1 - alpha_delta) exp(-w bearing) + alpha_delta exp(-0.07 magnitude)
//   score     = (1 - u + 0.01) wind + 0.5 u + 0.05 exp(-0.001 |level - 180|)
// evaluated left to right with no contraction.  A level whose triple is exactly (0, 1, 1) is not valid (features.py:153-159): score 0,
// skipped.  The choice is the reference loop's first strict maximum from best = 0: every lane keeps the first strict maximum of its
// own levels (ascending, '>'), then the wave reduces by (larger score, on equal scores the lower level) -- the same level as the
// sequential loop, whatever the ownership.
#pragma once
#include "ble_physics.h"

namespace ble {

constexpr uint32_t kFlagAgentNoLevel = 1024u;   // BLE_FLAG_AGENT_NO_LEVEL
constexpr int kSeekerLevels = 361;              // 2 x 181 - 1 relative levels, centre 180 (wind_column_center)
constexpr int kSeekerCentre = 180;
constexpr int kSeekerFirstWind = 16;            // the first triple of the wind column in the 1099-vector

// 0.05 * exp(-0.001 * k), k = |level - 180| = 0 .. 180: the reference's hysteresis term, tabulated with the host libm's exp (the
// device exp may round the last bit differently)
__device__ __constant__ const double kSeekerHysteresis[181] = {
    0x1.999999999999ap-5, 0x1.9930cb78c154cp-5, 0x1.98c81828fd793p-5, 0x1.985f7fa371720p-5, 0x1.97f701e1426bcp-5,
    0x1.978e9edb9753cp-5, 0x1.9726568b98d84p-5, 0x1.96be28ea71674p-5, 0x1.965615f14d2eap-5, 0x1.95ee1d995a1b7p-5,
    0x1.95863fdbc7d98p-5, 0x1.951e7cb1c7d30p-5, 0x1.94b6d4148d2fdp-5, 0x1.944f45fd4cd59p-5, 0x1.93e7d2653d66ap-5,
    0x1.9380794597420p-5, 0x1.93193a979482cp-5, 0x1.92b2165470ff9p-5, 0x1.924b0c756a4a8p-5, 0x1.91e41cf3bfb04p-5,
    0x1.917d47c8b237cp-5, 0x1.91168ced84a22p-5, 0x1.90afec5b7b69ap-5, 0x1.9049660bdcc1ap-5, 0x1.8fe2f9f7f0961p-5,
    0x1.8f7ca819008b0p-5, 0x1.8f16706857fc4p-5, 0x1.8eb052df43fcbp-5, 0x1.8e4a4f7713561p-5, 0x1.8de466291688ap-5,
    0x1.8d7e96ee9fca6p-5, 0x1.8d18e1c10306ep-5, 0x1.8cb3469995decp-5, 0x1.8c4dc571afa72p-5, 0x1.8be85e42a9698p-5,
    0x1.8b831105dde2fp-5, 0x1.8b1dddb4a983fp-5, 0x1.8ab8c4486a6fcp-5, 0x1.8a53c4ba807c1p-5, 0x1.89eedf044d30cp-5,
    0x1.898a131f33c71p-5, 0x1.8925610499298p-5, 0x1.88c0c8ade3f31p-5, 0x1.885c4a147c6f5p-5, 0x1.87f7e531cc998p-5,
    0x1.879399ff401c2p-5, 0x1.872f687644510p-5, 0x1.86cb509048403p-5, 0x1.86675246bca00p-5, 0x1.86036d9313d48p-5,
    0x1.859fa26ec1eecp-5, 0x1.853bf0d33cacdp-5, 0x1.84d858b9fb794p-5, 0x1.8474da1c776a8p-5, 0x1.841174f42b425p-5,
    0x1.83ae293a936dep-5, 0x1.834af6e92e050p-5, 0x1.82e7ddf97ac98p-5, 0x1.8284de64fb277p-5, 0x1.8221f8253233ep-5,
    0x1.81bf2b33a4ad3p-5, 0x1.815c7789d8fa0p-5, 0x1.80f9dd2157297p-5, 0x1.80975bf3a8f20p-5, 0x1.8034f3fa59b19p-5,
    0x1.7fd2a52ef66d0p-5, 0x1.7f706f8b0dcf8p-5, 0x1.7f0e5308302a5p-5, 0x1.7eac4f9fef744p-5, 0x1.7e4a654bdf494p-5,
    0x1.7de8940594ea3p-5, 0x1.7d86dbc6a73c2p-5, 0x1.7d253c88aec80p-5, 0x1.7cc3b64545ba7p-5, 0x1.7c6248f607e2ep-5,
    0x1.7c00f49492b39p-5, 0x1.7b9fb91a85411p-5, 0x1.7b3e968180419p-5, 0x1.7add8cc3260cdp-5, 0x1.7a7c9bd91a9b7p-5,
    0x1.7a1bc3bd0386bp-5, 0x1.79bb04688807fp-5, 0x1.795a5dd550f84p-5, 0x1.78f9cffd08d04p-5, 0x1.78995ad95ba71p-5,
    0x1.7838fe63f732bp-5, 0x1.77d8ba968ac6ep-5, 0x1.77788f6ac7555p-5, 0x1.77187cda5f6cdp-5, 0x1.76b882df07390p-5,
    0x1.7658a1727481fp-5, 0x1.75f8d88e5eabbp-5, 0x1.7599282c7eb60p-5, 0x1.753990468f3bbp-5, 0x1.74da10d64c727p-5,
    0x1.747aa9d5742a3p-5, 0x1.741b5b3dc5ccfp-5, 0x1.73bc2509025e4p-5, 0x1.735d0730ec7acp-5, 0x1.72fe01af4857cp-5,
    0x1.729f147ddbc2fp-5, 0x1.72403f966e220p-5, 0x1.71e182f2c8720p-5, 0x1.7182de8cb5472p-5, 0x1.7124525e00cc4p-5,
    0x1.70c5de6078c29p-5, 0x1.7067828dec812p-5, 0x1.70093ee02cf47p-5, 0x1.6fab13510c9e1p-5, 0x1.6f4cffda5f944p-5,
    0x1.6eef0475fb818p-5, 0x1.6e91211db7a44p-5, 0x1.6e3355cb6cce1p-5, 0x1.6dd5a278f5640p-5, 0x1.6d7807202d5d8p-5,
    0x1.6d1a83baf2443p-5, 0x1.6cbd18432333cp-5, 0x1.6c5fc4b2a0d90p-5, 0x1.6c0289034d723p-5, 0x1.6ba5652f0ccddp-5,
    0x1.6b48592fc44adp-5, 0x1.6aeb64ff5ad80p-5, 0x1.6a8e8897b8f37p-5, 0x1.6a31c3f2c8aa5p-5, 0x1.69d5170a75988p-5,
    0x1.697881d8ace81p-5, 0x1.691c04575d510p-5, 0x1.68bf9e8077188p-5, 0x1.6863504dec110p-5, 0x1.680719b9af999p-5,
    0x1.67aafabdb69d8p-5, 0x1.674ef353f7940p-5, 0x1.66f303766a7f9p-5, 0x1.66972b1f08edep-5, 0x1.663b6a47cdf75p-5,
    0x1.65dfc0eab63e8p-5, 0x1.65842f01bfeffp-5, 0x1.6528b486eac18p-5, 0x1.64cd517437f27p-5, 0x1.647205c3aa4a5p-5,
    0x1.6416d16f46197p-5, 0x1.63bbb47111379p-5, 0x1.6360aec313047p-5, 0x1.6305c05f54668p-5, 0x1.62aae93fdfcb6p-5,
    0x1.6250295ec126bp-5, 0x1.61f580b605f22p-5, 0x1.619aef3fbd2d0p-5, 0x1.614074f5f75bcp-5, 0x1.60e611d2c687bp-5,
    0x1.608bc5d03e3e7p-5, 0x1.603190e87391bp-5, 0x1.5fd773157d16bp-5, 0x1.5f7d6c5172e61p-5, 0x1.5f237c966e9b3p-5,
    0x1.5ec9a3de8b53fp-5, 0x1.5e6fe223e5b04p-5, 0x1.5e1637609bd1cp-5, 0x1.5dbca38ecd5b6p-5, 0x1.5d6326a89b711p-5,
    0x1.5d09c0a828b74p-5, 0x1.5cb0718799526p-5, 0x1.5c57394112e6fp-5, 0x1.5bfe17cebc989p-5, 0x1.5ba50d2abf0a1p-5,
    0x1.5b4c194f445ccp-5, 0x1.5af33c3678304p-5, 0x1.5a9a75da87a20p-5, 0x1.5a41c635a14cfp-5, 0x1.59e92d41f5491p-5,
    0x1.5990aaf9b52b3p-5, 0x1.59383f5714044p-5, 0x1.58dfea5446618p-5, 0x1.5887abeb824b5p-5, 0x1.582f8416ff459p-5,
    0x1.57d772d0f64efp-5, 0x1.577f7813a1e06p-5, 0x1.572793d93ded0p-5, 0x1.56cfc61c07e1ap-5, 0x1.56780ed63ea44p-5,
    0x1.56206e0222940p-5
};

// the environment's part of the score (station_seeker_agent.py:160-172): bearing weight and alpha_delta
struct SeekerEnv { double bearing_weight, alpha_delta; };
BLE_FN SeekerEnv seeker_env(float d32) {
  BLE_NO_CONTRACT
  const double d = (double)d32;
  const double distance = (d * 250.0) / (1.0 - d);
  double coeff = (distance - 250.0) / (500.0 - 250.0);
  coeff = coeff < 0.0 ? 0.0 : (coeff > 1.0 ? 1.0 : coeff);          // np.clip (a NaN stays NaN)
  SeekerEnv e;
  e.bearing_weight = 0.6 + coeff * (0.45 - 0.6);
  e.alpha_delta = exp(-distance / 35.0);
  return e;
}

// altitude_score of one valid level (station_seeker_agent.py:117-186)
BLE_FN double seeker_score(float u32, float b32, float m32, int level, const SeekerEnv& e) {
  BLE_NO_CONTRACT
  const double unc = (double)u32;
  const double bearing = 0.0 + (double)b32 * (3.141592653589793 - 0.0);
  const double mag = (double)m32;
  const double magnitude = (mag * 30.0) / (1.0 - mag);
  const double wind = (1.0 - e.alpha_delta) * exp(-e.bearing_weight * bearing) + e.alpha_delta * exp(-0.07 * magnitude);
  const int k = level < kSeekerCentre ? kSeekerCentre - level : level - kSeekerCentre;
  return (1.0 - unc + 0.01) * wind + unc * 0.5 + kSeekerHysteresis[k];
}

BLE_FN bool f32_finite(float v) { return v - v == 0.0f; }

// One environment per wave (`lane` 0 .. 63 of it).  Returns the chosen level (-1: none valid, or a non-finite feature read by the
// score; *bad is then set).  scores: optional [361] doubles of this environment.
BLE_FN int seeker_best_level(const float* __restrict__ row, int lane, double* __restrict__ scores, bool* bad) {
  const float d32 = row[7];
  const SeekerEnv e = seeker_env(d32);
  bool nonfinite = !f32_finite(d32);
  double best = 0.0;
  int best_level = 0x7fffffff;                      // (none: larger than every level, so that it loses every tie)
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int level = lane + 64 * j;
    if (level < kSeekerLevels) {
      const float* t = row + kSeekerFirstWind + 3 * level;
      const float u = t[0], b = t[1], m = t[2];
      const bool valid = (m != 1.0f) || (b != 1.0f) || (u != 0.0f);
      double s = 0.0;
      if (valid) {
        nonfinite |= !(f32_finite(u) && f32_finite(b) && f32_finite(m));
        s = seeker_score(u, b, m, level, e);
        if (s > best) { best = s; best_level = level; }
      }
      if (scores != nullptr) scores[level] = s;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(best, off, 64);
    const int ol = __shfl_xor(best_level, off, 64);
    if (os > best || (os == best && ol < best_level)) { best = os; best_level = ol; }
  }
  *bad = __any(nonfinite) || best_level == 0x7fffffff;
  return *bad ? -1 : best_level;
}

// pick_action (station_seeker_agent.py:72-86)
BLE_FN uint8_t seeker_action(int level) { return level < 0 ? 1 : (level < kSeekerCentre ? 2 : (level > kSeekerCentre ? 0 : 1)); }

// eval_agent's per-step body for one environment that is not yet done (eval_lib.py:157-190).  distance: units.relative_distance,
// sqrt(x^2 + y^2) in float64 on the float32 state, not contracted.
BLE_FN bool within_radius(float x32, float y32, double radius_m) {
  BLE_NO_CONTRACT
  const double x = (double)x32, y = (double)y32;
  return sqrt(x * x + y * y) <= radius_m;
}

}  // namespace ble
