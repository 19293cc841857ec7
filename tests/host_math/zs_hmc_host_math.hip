// The arithmetic and the index maps of Hamiltonian Monte Carlo (csrc/zs_hmc_math.h: __host__ __device__) compiled for the HOST
// and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_hmc_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) BEGIN / STEP / END over a grid of operands -- g = 0, p = 0, large and tiny values, eps from 1e-8 to 10 -- against
// long-double restatements of the formulas of include/zs_hmc.h, bound |err| <= 2^-20 S (float) / 2^-48 S (double), S the sum of
// the absolute values of the terms added; (2) dH, the acceptance probability and the decision at dH = +-800 and non-finite
// values, and the dual-averaging recursion, against long double to 2^-40 relative; (3) the chain-of-element map, the tile keys
// and the partial-sum slot map of k_hmc_move (zs_hmc.hip) over exactly-sized heap arrays for the layouts of
// tests/test_hmc_kernel.py: a host restatement of the kernel's tile loop, segmented scan included, must write every slot of the
// workspace exactly once and give every chain its sum.  Prints "hmc host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <limits>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_hmc_math.h"
#include "zs_host_check.h"

template <typename T> static ld rel_bound() { return sizeof(T) == 4 ? ldexpl(1.0L, -20) : ldexpl(1.0L, -48); }
template <typename T>
static void near(T got, ld want, ld S, const char* what) {
  expect(isfinite((double)got) && fabsl((ld)got - want) <= rel_bound<T>() * S, what, (double)got, (double)want);
}

template <typename T>
static void check_moves() {
  const double vals[] = {0.0, 1e-6, -1e-3, 0.37, -1.0, 2.5, -40.0, 1e3};
  const double steps[] = {1e-8, 1e-3, 0.1, 1.0, 10.0};
  for (double ed : steps) {
    const zs::HmcStep<T> st = zs::hmc_step_of<T>(ed);
    const ld E = ed, H = 0.5L * E;
    for (double qd : vals) for (double gd : vals) for (double pd : vals) {
      const T q0 = (T)qd, g = (T)gd, z = (T)pd;
      const ld Q = q0, G = g, Z = z;
      {  // BEGIN
        T q, p;
        const T sq = zs::hmc_begin(q0, g, z, st, q, p);
        const ld Sp = fabsl(Z) + fabsl(H * G);
        near<T>(p, Z + H * G, Sp, "begin p");
        near<T>(q, Q + E * (Z + H * G), fabsl(Q) + E * Sp, "begin q");
        near<T>(sq, Z * Z, Z * Z, "begin p0^2");
      }
      {  // STEP
        T q = q0, p = z;
        zs::hmc_step(q, p, g, st);
        const ld Sp = fabsl(Z) + fabsl(E * G);
        near<T>(p, Z + E * G, Sp, "step p");
        near<T>(q, Q + E * (Z + E * G), fabsl(Q) + E * Sp, "step q");
      }
      {  // END
        const T sq = zs::hmc_end(z, g, st);
        const ld Sp = fabsl(Z) + fabsl(H * G), P = Z + H * G;
        near<T>(sq, P * P, Sp * Sp, "end pL^2");
      }
    }
  }
}

static bool close40(double got, ld want) {
  if (!isfinite((double)want)) return got == (double)want;
  return fabsl((ld)got - want) <= ldexpl(1.0L, -40) * fabsl(want) + 1e-320L;
}

static void check_decide() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double lps[] = {0.0, -3.5, 12.25, -800.0, 800.0, 1e6, inf, -inf, nan};
  const double ks[] = {0.0, 0.5, 37.0, 800.0, inf, nan};
  const double us[] = {5.9604644775390625e-08, 1e-3, 0.5, 0.99999994039535522461, 1e-300};
  for (double l0 : lps) for (double l1 : lps) for (double k0 : ks) for (double k1 : ks) {
    const double dh = zs::hmc_delta_h(l0, l1, k0, k1);
    const ld want = ((ld)l1 - (ld)l0) - ((ld)k1 - (ld)k0);
    const bool fin = isfinite(l0) && isfinite(l1) && isfinite(k0) && isfinite(k1);
    expect(zs::hmc_finite(dh) == fin, "finite(dH)", zs::hmc_finite(dh), fin);
    const double a = zs::hmc_accept_prob(dh);
    if (!fin) {
      expect(a == 0.0, "a of a non-finite dH", a, 0.0);
      for (double u : us) expect(!zs::hmc_accept(dh, u), "a non-finite dH rejects", 1, 0);
      continue;
    }
    expect(close40(dh, want), "dH", dh, (double)want);
    expect(close40(a, expl(want < 0 ? want : 0.0L)) && a >= 0.0 && a <= 1.0, "a", a, (double)expl(want < 0 ? want : 0.0L));
    for (double u : us) {
      const ld lu = logl((ld)u);
      if (fabsl(lu - want) > 1e-9L * (1.0L + fabsl(want))) expect(zs::hmc_accept(dh, u) == (lu < want), "accept", zs::hmc_accept(dh, u), lu < want);
    }
  }
  for (double d : {800.0, -800.0}) {
    expect(zs::hmc_accept_prob(d) == (d > 0 ? 1.0 : 0.0), "a at +-800", zs::hmc_accept_prob(d), d > 0);
    expect(zs::hmc_accept(d, 0.5) == (d > 0), "accept at +-800", zs::hmc_accept(d, 0.5), d > 0);
  }
  // dual averaging: 400 adapting decides, then frozen ones; and a block that never adapted
  for (double e0 : {1e-8, 0.01, 1.0, 10.0}) {
    double st[ZS_HMC_STATE_DOUBLES] = {e0, e0, 0, 0, 0, 0, 0, 0};
    ld m = 0, hbar = 0, le = 0, leb = 0, eps = e0;
    const double delta = 0.8, gamma = 0.05, t0 = 100.0, kappa = 0.75;
    zs::hmc_adapt(st, 0.3, 0, delta, gamma, t0, kappa);
    expect(st[zs::HMC_EPS] == e0 && st[zs::HMC_M] == 0.0, "never adapted: eps unchanged", st[zs::HMC_EPS], e0);
    for (int it = 0; it < 400; ++it) {
      const double abar = it < 5 ? 0.0 : 0.5 + 0.5 * sin(0.37 * it);
      zs::hmc_adapt(st, abar, 1, delta, gamma, t0, kappa);
      m += 1;
      hbar = (1 - 1 / (m + t0)) * hbar + (delta - abar) / (m + t0);
      le = logl(10.0L * e0) - sqrtl(m) / gamma * hbar;
      const ld eta = powl(m, -kappa);
      leb = eta * le + (1 - eta) * leb;
      eps = expl(le);
      expect(fabsl(st[zs::HMC_EPS] - eps) <= ldexpl(1.0L, -40) * eps * (1 + fabsl(le)), "adapting eps", st[zs::HMC_EPS], (double)eps);
      expect(fabsl(st[zs::HMC_LOG_EPSBAR] - leb) <= ldexpl(1.0L, -40) * (1 + fabsl(leb)), "log epsbar", st[zs::HMC_LOG_EPSBAR], (double)leb);
      expect(st[zs::HMC_M] == (double)m, "m", st[zs::HMC_M], (double)m);
    }
    for (int it = 0; it < 3; ++it) {
      zs::hmc_adapt(st, 0.1, 0, delta, gamma, t0, kappa);
      expect(fabsl(st[zs::HMC_EPS] - expl(leb)) <= ldexpl(1.0L, -40) * expl(leb) * (1 + fabsl(leb)), "frozen eps", st[zs::HMC_EPS], (double)expl(leb));
      expect(st[zs::HMC_M] == 400.0, "frozen m", st[zs::HMC_M], 400.0);
    }
  }
}

// Host restatement of the tile loop of k_hmc_move (zs_hmc.hip) for C chains of tensors with these rows: exactly-sized heap
// arrays, so that a read or write outside a tensor or the workspace is an AddressSanitizer report.  The data are small
// integers, so every order of summation gives the same float.
static void walk_layout(int64_t C, const std::vector<int64_t>& rows) {
  const int nt = (int)rows.size();
  std::vector<int64_t> start(nt + 1, 0), poff(nt + 1, 0);
  for (int s = 0; s < nt; ++s) {
    start[s + 1] = start[s] + C * rows[s];
    poff[s + 1] = poff[s] + zs::hmc_pieces(rows[s]);
  }
  const int64_t n = start[nt], slots = poff[nt], tiles = (n + ZS_HMC_TILE - 1) / ZS_HMC_TILE;
  std::vector<std::vector<float>> val(nt);
  std::vector<double> want(C, 0.0);
  for (int s = 0; s < nt; ++s) {
    val[s].resize(C * rows[s]);
    for (int64_t k = 0; k < C * rows[s]; ++k) {
      val[s][k] = (float)((start[s] + k) % 7);
      want[k / rows[s]] += val[s][k];
    }
  }
  std::vector<float> ksum(C * slots, -1.0f);
  std::vector<int> writes(C * slots, 0);
  std::vector<float> a(ZS_HMC_TILE), b(ZS_HMC_TILE);
  std::vector<int> key(ZS_HMC_TILE);
  for (int64_t tile = 0; tile < tiles; ++tile) {
    int prev = -2;
    for (int e = 0; e < ZS_HMC_TILE; ++e) {
      const int64_t i = tile * ZS_HMC_TILE + e;
      if (i >= n) { a[e] = 0.0f; key[e] = 1 << 30; continue; }
      const int64_t gi = i >> 2;
      const int64_t ci = zs::flat_clamped_index(gi, (int)(i & 3), n);
      expect(ci == i && zs::flat_element_live(gi, (int)(i & 3), n), "a live element is its own clamped index", (double)ci, (double)i);
      const zs::HmcLoc l = zs::hmc_locate(start.data(), rows.data(), nt, i);
      expect(l.s >= 0 && l.s < nt && l.off >= 0 && l.off < C * rows[l.s] && l.chain == l.off / rows[l.s] && l.chain < C &&
                 l.run_start == start[l.s] + l.chain * rows[l.s],
             "element inside its tensor and chain", (double)l.off, (double)l.s);
      a[e] = val[l.s].at(l.off);
      key[e] = zs::hmc_key(l.run_start, tile);
      expect(key[e] >= prev && key[e] >= -1 && key[e] <= e, "keys ascend inside a tile", key[e], prev);
      prev = key[e];
    }
    for (int d = 1; d < ZS_HMC_TILE; d <<= 1) {
      for (int e = 0; e < ZS_HMC_TILE; ++e) b[e] = a[e] + ((e >= d && key.at(e - d) == key[e]) ? a[e - d] : 0.0f);
      a.swap(b);
    }
    for (int e = 0; e < ZS_HMC_TILE; ++e) {
      const int64_t i = tile * ZS_HMC_TILE + e;
      if (i < n && (e == ZS_HMC_TILE - 1 || i + 1 >= n || key.at(e + 1) != key[e])) {
        const zs::HmcLoc l = zs::hmc_locate(start.data(), rows.data(), nt, i);
        const int64_t slot = zs::hmc_slot(l.chain, slots, poff[l.s], l.run_start, tile);
        expect(slot >= l.chain * slots + poff[l.s] && slot < l.chain * slots + poff[l.s + 1], "slot inside its tensor's slots", (double)slot, 0);
        ksum.at(slot) = a[e];
        ++writes.at(slot);
        const int64_t r = rows[l.s];
        if (i == l.run_start + r - 1 && zs::hmc_pieces_of(l.run_start, r) < zs::hmc_pieces(r)) {
          ksum.at(slot + 1) = 0.0f;
          ++writes.at(slot + 1);
          expect(slot + 1 < l.chain * slots + poff[l.s + 1], "zero slot inside its tensor's slots", (double)slot, 0);
        }
      }
    }
  }
  for (int64_t c = 0; c < C; ++c) {
    double got = 0.0;
    for (int64_t j = 0; j < slots; ++j) {
      expect(writes[c * slots + j] == 1, "every slot written exactly once", writes[c * slots + j], 1);
      got += ksum[c * slots + j];
    }
    expect(got == want[c], "a chain's slots add up to its sum", got, want[c]);
  }
}

int main() {
  check_moves<float>();
  check_moves<double>();
  check_decide();
  const int64_t Cs[] = {1, 3, 64, 65, 257}, rows[] = {1, 3, 4, 5, 63, 64, 65, 257, 4099};
  for (int64_t C : Cs) for (int64_t r : {1, 5, 64}) walk_layout(C, {r});
  for (int64_t r : rows) for (int64_t C : {1, 3}) walk_layout(C, {r});
  walk_layout(1, {(1 << 20) + 5});
  for (int64_t C : {1, 3, 65}) {
    walk_layout(C, {5, 7});
    walk_layout(C, {8, 12});
    walk_layout(C, std::vector<int64_t>(32, 4));
    walk_layout(C, {1023, 1025, 2, 2047});
  }
  return finish("hmc host math ok");
}
