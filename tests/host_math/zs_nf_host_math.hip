// The arithmetic and the lane map of the planar / Householder flow kernels (csrc/zs_nf_math.h with zs_group_math.h: __host__
// __device__) compiled for the HOST and run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_nf_host_math.py):
//     hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined ...
// (1) the parameter formulas (s in {-30, -3, 0, 3, 30}), one planar layer with its backward pieces and the parameter chain
//     (|a| up to 20), one reflection with its backward, in the kernels' own order (the *_row restatements of zs_nf_math.h), against
//     long double for every D of tests/test_nf_kernel.py; every operand sits in an exactly-sized heap array;
// (2) the lane-group and row-tile maps, the LDS places of z_l and t_l and the places of the partial sums for every D,
//     R in {1, 3, 65} and L in {1, 32}: a group never crosses its wave, every (row, i, l) is owned exactly once, every LDS place
//     of a tile is its owner's alone and inside the exactly-sized array, every partials element is written exactly once.
// Prints "nf host math ok: N checks".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../zhusuan-pytorch_amd/csrc/zs_nf_math.h"
#include "zs_host_check.h"

// 2^-20 (2^-48) of the summed term magnitudes: the unit of a result through a library function (tests/README_nf.md)
template <typename T> static ld lib_unit() { return sizeof(T) == 4 ? ldexpl(1.0L, -20) : ldexpl(1.0L, -48); }
template <typename T> static void close(const char* what, T got, ld want, ld mag, int D) {
  expect(isfinite((double)got) && fabsl((ld)got - want) <= (D + 8) * lib_unit<T>() * mag, what, (double)got, (double)want);
}

static const int Ds[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 40, 63, 64};

static ld dotl(const std::vector<ld>& a, const std::vector<ld>& b, ld* mag = nullptr) {
  ld s = 0, m = 0;
  for (size_t d = 0; d < a.size(); ++d) { s += a[d] * b[d]; m += fabsl(a[d] * b[d]); }
  if (mag) *mag = m;
  return s;
}
template <typename T> static T* heap(int n) { return (T*)malloc(sizeof(T) * (n > 0 ? n : 1)); }
template <typename T> static std::vector<ld> wide(const T* a, int n) { return std::vector<ld>(a, a + n); }

// ---------------------------------------------------------------- (1)
template <typename T>
static void check_arithmetic() {
  const double S[] = {-30, -3, 0, 3, 30}, A[] = {-20, -5, -0.5, 0, 0.5, 5, 20};
  for (int D : Ds) for (double s_target : S) {
    T *u = heap<T>(D), *w = heap<T>(D), *uh = heap<T>(D), *z = heap<T>(D), *z0 = heap<T>(D), *g = heap<T>(D), *g0 = heap<T>(D);
    T *Guh = heap<T>(D), *Gw = heap<T>(D), *gu = heap<T>(D), *gw = heap<T>(D), *v = heap<T>(D), *gv = heap<T>(D);
    double wu = 0, ww = 0;
    for (int d = 0; d < D; ++d) { w[d] = (T)(normal01() / sqrt((double)D)); u[d] = (T)(normal01() / sqrt((double)D)); }
    for (int d = 0; d < D; ++d) { wu += (double)w[d] * (double)u[d]; ww += (double)w[d] * (double)w[d]; }
    for (int d = 0; d < D; ++d) u[d] = (T)((double)u[d] + (s_target - wu) * (double)w[d] / ww);
    // the parameter quantities
    const zs::NfParams<T> p = zs::nf_planar_params_row(u, w, uh, D);
    const std::vector<ld> ul = wide(u, D), wl = wide(w, D);
    ld smag, nl, cmag;
    const ld sl = dotl(wl, ul, &smag);
    nl = dotl(wl, wl);
    const ld spl = fmaxl(sl, 0) + log1pl(expl(-fabsl(sl))), kl = spl - 1 - sl;
    std::vector<ld> uhl(D);
    for (int d = 0; d < D; ++d) uhl[d] = ul[d] + kl * wl[d] / nl;
    const ld cl = dotl(wl, uhl, &cmag);
    const ld kmag = spl + 1 + fabsl(sl) + 2 * smag;          // k moves by at most 2 e_s
    close<T>("s", p.s, sl, smag, D);
    close<T>("n", p.n, nl, nl, D);
    close<T>("k", p.k, kl, kmag, D);
    ld uhmag = 0;
    for (int d = 0; d < D; ++d) {
      const ld qmag = fabsl(wl[d]) * kmag / nl + fabsl(kl * wl[d] / nl) * 2;
      close<T>("uh", uh[d], uhl[d], fabsl(ul[d]) + qmag, D);
      uhmag += fabsl(wl[d]) * (fabsl(ul[d]) + qmag);
    }
    close<T>("c", p.c, cl, cmag + (D + 8) * uhmag, D);
    close<T>("c = softplus(s) - 1", p.c, spl - 1, cmag + (D + 8) * uhmag, D);
    close<T>("dk", zs::nf_planar_dk(p.s), -1 / (1 + expl(sl)), 2 + smag, D);
    if (fabs(s_target) > 3) {          // 1 + h c may vanish in T at s = -30: the layer is checked where it is well conditioned
      free(u); free(w); free(uh); free(z); free(z0); free(g); free(g0); free(Guh); free(Gw); free(gu); free(gw); free(v); free(gv);
      continue;
    }
    for (double a_target : A) {
      // one layer: b is chosen so that a = w.z + b hits the target
      for (int d = 0; d < D; ++d) { z0[d] = z[d] = (T)(2.0 * normal01()); g0[d] = g[d] = (T)normal01(); Guh[d] = (T)normal01(); Gw[d] = (T)normal01(); }
      const std::vector<ld> zl = wide(z0, D), gl = wide(g0, D), Gul = wide(Guh, D), Gwl = wide(Gw, D);
      ld amag;
      const ld wz = dotl(wl, zl, &amag);
      const T b = (T)(a_target - (double)wz), gld = (T)normal01();
      T ldet = (T)0.25;
      const T t = zs::nf_planar_layer_row(w, b, uh, p.c, z, &ldet, D);
      const ld al = wz + (ld)b, tl = tanhl(al), hl = 1 - tl * tl, ml = 1 + hl * (ld)p.c;
      amag += fabsl((ld)b);
      close<T>("t", t, tl, 1 + amag, D);
      const ld e_t = (D + 8) * lib_unit<T>() * (1 + amag);
      for (int d = 0; d < D; ++d)
        close<T>("z'", z[d], zl[d] + (ld)uh[d] * tl, fabsl(zl[d]) + fabsl((ld)uh[d]) * (1 + (D + 8) * (1 + amag)), D);
      close<T>("logdet", ldet, 0.25L + logl(fabsl(ml)), 0.25L + fabsl(logl(fabsl(ml))) + (1 + (D + 8) * (1 + amag) * 2 * fabsl((ld)p.c)) / fabsl(ml), D);
      // its backward at the kernel's own t (the pieces are functions of t, c, uh as computed)
      const ld tt = t, ht = 1 - tt * tt, mt = 1 + ht * (ld)p.c;
      T Gb = (T)0.5, Gc = (T)-0.5;
      zs::nf_planar_layer_bwd_row(w, uh, p.c, t, z0, gld, g, Guh, Gw, &Gb, &Gc, D);
      ld gmag;
      const ld dg = dotl(gl, wide(uh, D), &gmag);
      const ld t2 = (ld)gld * ((ld)p.c / mt) * (-2 * tt), gal = (dg + t2) * ht, gamag = (gmag + 2 * fabsl(t2)) + fabsl(gal);
      close<T>("Gb", Gb, 0.5L + gal, 0.5L + gamag, D);
      close<T>("Gc", Gc, -0.5L + (ld)gld * ht / mt, 0.5L + 2 * fabsl((ld)gld * ht / mt), D);
      for (int d = 0; d < D; ++d) {
        close<T>("Guh", Guh[d], Gul[d] + gl[d] * tt, fabsl(Gul[d]) + fabsl(gl[d]), D);
        close<T>("Gw", Gw[d], Gwl[d] + gal * zl[d], fabsl(Gwl[d]) + gamag * fabsl(zl[d]), D);
        close<T>("g", g[d], gl[d] + gal * wl[d], fabsl(gl[d]) + gamag * fabsl(wl[d]), D);
      }
      (void)e_t;
      // the parameter chain of P1f from those sums
      const std::vector<ld> Au = wide(Guh, D), Aw = wide(Gw, D);
      zs::nf_planar_finish_row(u, w, Guh, Gw, Gc, gu, gw, D);
      std::vector<ld> G1(D), W1(D);
      ld pmag;
      for (int d = 0; d < D; ++d) { G1[d] = Au[d] + (ld)Gc * wl[d]; W1[d] = Aw[d] + (ld)Gc * uhl[d]; }
      const ld pl = dotl(G1, wl, &pmag), dkl = -1 / (1 + expl(sl));
      for (int d = 0; d < D; ++d) {
        const ld mg = fabsl(G1[d]) + fabsl(W1[d]) + (pmag / nl) * (fabsl(wl[d]) + fabsl(ul[d])) * (1 + smag) + fabsl(G1[d]) * kmag / nl +
                      2 * kmag * pmag / (nl * nl) * fabsl(wl[d]) * 3 + fabsl((ld)Gc) * (fabsl(ul[d]) + kmag * fabsl(wl[d]) / nl * 3);
        close<T>("gu", gu[d], G1[d] + (pl / nl) * dkl * wl[d], (D + 8) * mg, D);
        close<T>("gw", gw[d], W1[d] + G1[d] * kl / nl + (pl / nl) * dkl * ul[d] - 2 * kl * pl / (nl * nl) * wl[d], (D + 8) * mg, D);
      }
    }
    // one reflection and its backward
    for (int d = 0; d < D; ++d) { v[d] = (T)normal01(); z0[d] = z[d] = (T)(2.0 * normal01()); g0[d] = g[d] = (T)normal01(); }
    const std::vector<ld> vl = wide(v, D), zl = wide(z0, D), gl = wide(g0, D);
    ld pm, qm;
    const ld nn = dotl(vl, vl), pp = dotl(vl, zl, &pm), qq = dotl(vl, gl, &qm);
    zs::nf_householder_layer_row(v, z, D);
    zs::nf_householder_layer_bwd_row(v, z0, g, gv, D);
    for (int d = 0; d < D; ++d) {
      close<T>("reflection", z[d], zl[d] - 2 * vl[d] * pp / nn, fabsl(zl[d]) + 4 * fabsl(vl[d]) * pm / nn, D);
      close<T>("reflected cotangent", g[d], gl[d] - 2 * vl[d] * qq / nn, fabsl(gl[d]) + 4 * fabsl(vl[d]) * qm / nn, D);
      close<T>("gv", gv[d], -2 * (pp * gl[d] + qq * zl[d]) / nn + 4 * pp * qq * vl[d] / (nn * nn),
               4 * (pm * fabsl(gl[d]) + qm * fabsl(zl[d])) / nn + 12 * pm * qm * fabsl(vl[d]) / (nn * nn), D);
    }
    free(u); free(w); free(uh); free(z); free(z0); free(g); free(g0); free(Guh); free(Gw); free(gu); free(gw); free(v); free(gv);
  }
  expect(zs::nf_planar_z<T>((T)5, (T)2, (T)1.5) == (T)8 && zs::nf_planar_h<T>((T)0.5) == (T)0.75 && zs::nf_planar_m<T>((T)0.75, (T)2) == (T)2.5, "steps", 0, 0);
  expect(zs::nf_householder_z<T>((T)5, (T)1, (T)3, (T)2) == (T)2 && zs::nf_planar_g<T>((T)1, (T)2, (T)3) == (T)7, "steps", 0, 0);
  expect(zs::nf_softplus<T>((T)0) == (T)logl(2.0L) && zs::nf_planar_dk<T>((T)0) == (T)-0.5, "softplus and dk at 0", 0, 0);
}

// ---------------------------------------------------------------- (2)
static void check_maps() {
  const int64_t Rs[] = {1, 3, 65};
  const int Ls[] = {1, 32};
  expect(zs::group_lanes(0) == 1 && zs::group_lanes(65) == 64, "group lanes at the edges", 0, 0);
  expect(zs::nf_workgroups(1, 64) == 1 && zs::nf_workgroups(65, 64) == 65 && zs::nf_workgroups(65, 4) == 5 &&
         zs::nf_workgroups((int64_t)1 << 40, 1) == ZS_NF_MAX_WORKGROUPS, "workgroups", 0, 0);
  for (int D : Ds) {
    const int G = zs::group_lanes(D);
    expect(G >= D && (G == 1 || G / 2 < D) && (G & (G - 1)) == 0 && G <= 64, "group lanes", G, D);
    for (int64_t R : Rs) for (int L : Ls) {
      const int own = zs::nf_workgroups(R, G);
      const int grids[] = {own, 1, 3};          // the library's own grid, and capped ones that walk several tiles
      for (int blocks : grids) {
        unsigned char* owned = (unsigned char*)calloc((size_t)(R * D * L), 1);                                   // (row, i, l)
        unsigned char* part = (unsigned char*)calloc((size_t)zs::nf_partial_row(blocks, 0, D, L), 1);            // exactly sized
        const int64_t n_lds = zs::nf_planar_bwd_lds(D, L, G), z_at = n_lds - zs::nf_householder_bwd_lds(L), t_at = (int64_t)L * D + L;
        for (int b = 0; b < blocks; ++b) {
          bool first_tile = true;
          const zs::GroupPlace p0 = zs::group_place(0, ZS_NF_THREADS, G);
          for (int64_t rb = zs::group_row_first(b, p0); rb < R; rb += zs::group_row_step(blocks, p0), first_tile = false) {
            unsigned char* lds = (unsigned char*)calloc((size_t)n_lds, 1);          // one tile's writes
            for (int tid = 0; tid < ZS_NF_THREADS; ++tid) {
              const zs::GroupPlace pl = zs::group_place(tid, ZS_NF_THREADS, G);
              expect(pl.lane >= 0 && pl.lane < G && pl.first % G == 0 && pl.first + G <= 64 && tid - pl.first == pl.lane && pl.grp == pl.first / G &&
                     pl.groups * G == 64, "a group stays inside its wave", pl.first, pl.lane);
              const int64_t r = rb + pl.grp;
              for (int l = 0; l < L; ++l) {
                ++lds[z_at + zs::nf_z_index(l, tid)];
                if (pl.lane == 0) ++lds[t_at + zs::nf_t_index(l, pl.grp, pl.groups)];
                if (pl.lane < D && tid < D) ++lds[(int64_t)l * D + tid];          // uh_l[d] by lane d of the wave
                if (tid == 0) ++lds[(int64_t)L * D + l];                        // c_l
                if (r < R && pl.lane < D) ++owned[(r * D + pl.lane) * L + l];
                if (first_tile) {
                  const int64_t P = zs::nf_partial_row(b, l, D, L);
                  if (pl.grp == 0 && pl.lane < D) { ++part[P + zs::nf_partial_guh(pl.lane)]; ++part[P + zs::nf_partial_gw(pl.lane, D)]; }
                  if (tid == 0) { ++part[P + zs::nf_partial_gb(D)]; ++part[P + zs::nf_partial_gc(D)]; }
                }
              }
            }
            bool once = true;
            for (int64_t i = 0; i < n_lds; ++i) once = once && lds[i] == 1;
            expect(once, "every LDS place of a tile has one owner and none is idle", D, (double)L);
            free(lds);
          }
        }
        bool once = true;
        for (int64_t i = 0; i < R * D * L; ++i) once = once && owned[i] == 1;
        expect(once, "every (row, i, l) owned exactly once", D, (double)R);
        once = true;
        for (int64_t i = 0; i < zs::nf_partial_row(blocks, 0, D, L); ++i) once = once && part[i] == 1;
        expect(once || blocks > own, "every partials element written exactly once", D, (double)R);
        free(owned); free(part);
      }
    }
  }
}

int main() {
  check_arithmetic<float>();
  check_arithmetic<double>();
  check_maps();
  return finish("nf host math ok");
}
