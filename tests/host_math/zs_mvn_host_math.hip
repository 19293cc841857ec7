// The arithmetic and the lane map of the multivariate-normal kernels (csrc/zs_mvn_math.h with zs_group_math.h: __host__ __device__)
// compiled for the HOST and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_mvn_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) the matvec and the two substitutions in the kernels' own order (mvn_matvec_row, mvn_forward_row, mvn_backward_row: the
//     steps the lanes of a group make together) and the density against long double for every D of tests/test_mvn_kernel.py,
//     on that test's recipe for L (diagonal U[0.5, 2], strict lower part N(0, 1) 0.5 / sqrt(D)), to that test's bounds; L sits in
//     an exactly-sized heap array whose upper triangle is NaN, so a read of it would show;
// (2) the lane-group map for every D and R in {1, 3, 65}: a group never crosses its wave, every (row, i) is owned exactly once,
//     the walk of a group over a D x D matrix touches every element exactly once and stays inside the exactly-sized array, and the
//     LDS tile indices of a wave's lower triangles are distinct and inside the tile.   Prints "mvn host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_mvn_math.h"
#include "zs_host_check.h"

template <typename T> static ld unit() { return sizeof(T) == 4 ? ldexpl(1.0L, -24) : ldexpl(1.0L, -53); }

static const int Ds[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64};

// |L^-1| (lower triangular, long double), row-major D x D
static std::vector<ld> abs_inverse(const std::vector<ld>& L, int D) {
  std::vector<ld> inv((size_t)D * D, 0);
  for (int c = 0; c < D; ++c)
    for (int i = c; i < D; ++i) {
      ld s = i == c ? 1 : 0;
      for (int j = c; j < i; ++j) s -= L[i * D + j] * inv[j * D + c];
      inv[i * D + c] = s / L[i * D + i];
    }
  for (ld& v : inv) v = fabsl(v);
  return inv;
}

// ---------------------------------------------------------------- (1)
template <typename T>
static void check_arithmetic() {
  const ld u = unit<T>();
  for (int D : Ds) for (int rep = 0; rep < 6; ++rep) {
    T* L = (T*)malloc(sizeof(T) * D * D);          // exactly sized, NaN above the diagonal
    T* mean = (T*)malloc(sizeof(T) * D);
    T* x = (T*)malloc(sizeof(T) * D);
    T* e = (T*)malloc(sizeof(T) * D);
    T* z = (T*)malloc(sizeof(T) * D);
    T* y = (T*)malloc(sizeof(T) * D);
    T* w = (T*)malloc(sizeof(T) * D);
    std::vector<ld> Ll((size_t)D * D, 0);
    for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) {
      L[i * D + j] = j > i ? (T)NAN : j == i ? (T)(0.5 + 1.5 * uniform01()) : (T)(normal01() * 0.5 / sqrt((double)D));
      if (j <= i) Ll[i * D + j] = (ld)L[i * D + j];
    }
    for (int i = 0; i < D; ++i) {
      mean[i] = (T)(3.0 * normal01());
      x[i] = (T)((double)mean[i] + 2.0 * normal01());
      e[i] = (T)normal01();
    }
    const std::vector<ld> Li = abs_inverse(Ll, D);
    // matvec
    zs::mvn_matvec_row(L, D, mean, e, z, D);
    for (int i = 0; i < D; ++i) {
      ld want = mean[i], mag = fabsl((ld)mean[i]);
      for (int j = 0; j <= i; ++j) { want += Ll[i * D + j] * (ld)e[j]; mag += fabsl(Ll[i * D + j] * (ld)e[j]); }
      expect(fabsl((ld)z[i] - want) <= (D + 2) * u * mag, "matvec", (double)z[i], (double)want);
    }
    // forward substitution
    std::vector<ld> yl(D), wl(D), ey(D), ew(D);
    for (int i = 0; i < D; ++i) {
      ld s = (ld)x[i] - (ld)mean[i];
      for (int j = 0; j < i; ++j) s -= Ll[i * D + j] * yl[j];
      yl[i] = s / Ll[i * D + i];
      y[i] = x[i] - mean[i];
    }
    zs::mvn_forward_row(L, D, y, D);
    for (int i = 0; i < D; ++i) {
      ey[i] = 0;
      for (int c = 0; c <= i; ++c) {
        ld inner = fabsl((ld)x[c]) + fabsl((ld)mean[c]);
        for (int j = 0; j <= c; ++j) inner += fabsl(Ll[c * D + j]) * fabsl(yl[j]);
        ey[i] += Li[i * D + c] * inner;
      }
      ey[i] *= (D + 3) * u;
      expect(isfinite((double)y[i]) && fabsl((ld)y[i] - yl[i]) <= ey[i], "forward substitution", (double)y[i], (double)yl[i]);
    }
    // back substitution at the rounded y's exact preimage: w = L^-T y_true, the kernel solves from its own y
    for (int i = D - 1; i >= 0; --i) {
      ld s = yl[i];
      for (int j = i + 1; j < D; ++j) s -= Ll[j * D + i] * wl[j];
      wl[i] = s / Ll[i * D + i];
      w[i] = y[i];
    }
    zs::mvn_backward_row(L, D, w, D);
    for (int i = 0; i < D; ++i) {
      ew[i] = 0;
      for (int c = i; c < D; ++c) {          // |L^-T|_ic = |L^-1|_ci
        ld inner = 0;
        for (int j = c; j < D; ++j) inner += fabsl(Ll[j * D + c]) * fabsl(wl[j]);
        ew[i] += Li[c * D + i] * ((D + 3) * u * inner + ey[c]);
      }
      expect(isfinite((double)w[i]) && fabsl((ld)w[i] - wl[i]) <= ew[i], "back substitution", (double)w[i], (double)wl[i]);
    }
    // density from the kernel's y: sum_i log L_ii and sum_i y_i^2 in ascending i stand for the group's butterflies
    T slog = 0, ss = 0;
    ld slogl = 0, ssl = 0, sabs = 0, lin = 0;
    for (int i = 0; i < D; ++i) {
      slog += zs::mvn_log(L[i * D + i]);
      ss += y[i] * y[i];
      slogl += logl(Ll[i * D + i]);
      sabs += fabsl(logl(Ll[i * D + i]));
      ssl += yl[i] * yl[i];
      lin += fabsl(yl[i]) * ey[i];
    }
    const ld c0 = -0.5L * D * logl(6.283185307179586476925286766559L);
    const T lp = zs::mvn_lp((T)c0, slog, ss);
    const ld want = c0 - slogl - 0.5L * ssl;
    expect(isfinite((double)lp) && fabsl((ld)lp - want) <= lin + (D + 4) * u * (0.5L * ssl + sabs - c0), "density", (double)lp, (double)want);
    // the gtril step
    const T acc = zs::mvn_gtril_step((T)0.25, (T)-1.5, w[0], y[0], true, zs::mvn_rdiag(L[0]));
    const ld wacc = 0.25L - 1.5L * ((ld)w[0] * (ld)y[0] - 1 / Ll[0]);
    expect(fabsl((ld)acc - wacc) <= 4 * u * (0.25L + 1.5L * (fabsl((ld)w[0] * (ld)y[0]) + 1 / Ll[0])), "gtril step", (double)acc, (double)wacc);
    free(L); free(mean); free(x); free(e); free(z); free(y); free(w);
  }
  expect(zs::mvn_lp<T>((T)1, (T)2, (T)4) == (T)-3, "lp", 0, 0);
  expect(zs::mvn_subst_step<T>((T)5, (T)2, (T)1.5) == (T)2 && zs::mvn_matvec_step<T>((T)5, (T)2, (T)1.5) == (T)8, "steps", 0, 0);
}

// ---------------------------------------------------------------- (2)
static void check_lane_groups() {
  const int64_t Rs[] = {1, 3, 65};
  expect(zs::group_lanes(0) == 1 && zs::group_lanes(65) == 64, "group lanes at the edges", 0, 0);
  for (int D : Ds) {
    const int G = zs::group_lanes(D);
    expect(G >= D && (G == 1 || G / 2 < D) && (G & (G - 1)) == 0 && G <= 64, "group lanes", G, D);
    // the wave's tile: every (group, i >= j) has its own place inside it
    std::vector<unsigned char> tile((size_t)zs::mvn_tile_elements(G), 0);          // .at() checks the bound
    for (int grp = 0; grp < ZS_MVN_THREADS / G; ++grp)
      for (int i = 0; i < D; ++i) for (int j = 0; j <= i; ++j) ++tile.at((size_t)zs::mvn_tile_index(grp, i, j, G));
    bool distinct = true;
    for (unsigned char c : tile) distinct = distinct && c <= 1;
    expect(distinct, "tile places are distinct", D, G);
    for (int64_t R : Rs) for (int blocks = 1; blocks <= 3; blocks += 2) {
      unsigned char* owned = (unsigned char*)calloc((size_t)(R * D), 1);            // (row, i)
      unsigned char* touched = (unsigned char*)calloc((size_t)(R * D * D), 1);      // (row, i, j) of the walk
      unsigned char* lower = (unsigned char*)calloc((size_t)(R * D * D), 1);        // (row, i >= j) read on the way in
      for (int b = 0; b < blocks; ++b) for (int tid = 0; tid < ZS_MVN_THREADS; ++tid) {
        const zs::GroupPlace pl = zs::group_place(tid, ZS_MVN_THREADS, G);
        expect(pl.lane >= 0 && pl.lane < G && pl.first % G == 0 && pl.first + G <= 64 && tid - pl.first == pl.lane && pl.grp == pl.first / G &&
               pl.groups * G == 64, "a group stays inside its wave", pl.first, pl.lane);
        for (int64_t rb = zs::group_row_first(b, pl); rb < R; rb += zs::group_row_step(blocks, pl)) {
          const int64_t r = rb + pl.grp;
          if (r >= R) continue;
          if (pl.lane < D) ++owned[r * D + pl.lane];
          for (zs::MvnWalk w = zs::mvn_walk_first(pl.lane, D); w.i < D; zs::mvn_walk_next(w, G, D)) {
            expect(w.j >= 0 && w.j < D, "the walk stays inside a row", w.j, D);
            ++touched[(r * D + w.i) * D + w.j];
            if (w.j <= w.i) ++lower[(r * D + w.i) * D + w.j];
          }
        }
      }
      bool once = true;
      for (int64_t i = 0; i < R * D; ++i) once = once && owned[i] == 1;
      expect(once, "every (row, i) owned exactly once", D, (double)R);
      once = true;
      for (int64_t i = 0; i < R * D * D; ++i) once = once && touched[i] == 1;
      expect(once, "every element of a row's matrix written exactly once", D, (double)R);
      once = true;
      for (int64_t r = 0; r < R; ++r) for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j)
        once = once && lower[(r * D + i) * D + j] == (j <= i ? 1 : 0);
      expect(once, "every (row, i >= j) read exactly once and nothing above the diagonal", D, (double)R);
      free(owned); free(touched); free(lower);
    }
  }
}

int main() {
  check_arithmetic<float>();
  check_arithmetic<double>();
  check_lane_groups();
  return finish("mvn host math ok");
}
