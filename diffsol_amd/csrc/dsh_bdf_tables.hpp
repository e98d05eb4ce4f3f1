// Bdf::_new tables (bdf.rs:286-306): alpha, gamma and the squared error constants of the orders 1..5, by ONE function that the host set-up of the
// device-resident BDF calls at run time (dsh_adaptive.hip) and that the per-order step bodies of the lock-step fast kernel evaluate at compile time
// (dsh_adaptive_kernel.hpp, kBdfTables): IEEE double operations in one order, nothing contracted (a constant evaluator never fuses; the set-up's translation
// unit is compiled with -ffp-contract=off), so both give the same 64-bit patterns.  tests/test_bdf_tables.py holds them to that on the host: the function run
// as compiled code against the constant-evaluated table.  Plain C++ without includes: hipcc, hiprtc and a host compiler all take it.
#pragma once

namespace dsh {

struct BdfTables {
  double alpha[6], gamma[6], ec2[6];
};

constexpr BdfTables bdf_new_tables() {
  BdfTables T{};
  const double kappa[6] = {0.0, -0.1850, -1.0 / 9.0, -0.0823, -0.0415, 0.0};
  T.alpha[0] = 0.0; T.gamma[0] = 0.0; T.ec2[0] = 1.0;
  for (int i = 1; i <= 5; ++i) {
    const double i_t = (double)i, one_over_i = 1.0 / i_t, one_over_i_plus_one = 1.0 / (i_t + 1.0);
    T.gamma[i] = T.gamma[i - 1] + one_over_i;
    T.alpha[i] = 1.0 / ((1.0 - kappa[i]) * T.gamma[i]);
    const double e = kappa[i] * T.gamma[i] + one_over_i_plus_one;
    T.ec2[i] = e * e;
  }
  return T;
}

inline constexpr BdfTables kBdfTables = bdf_new_tables();

}  // namespace dsh
