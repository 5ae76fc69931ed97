// tests/cpp/act_plan_check.cpp -- the LDS plans of the banded conv-stack kernel and the panelled row-block kernel (smarties_amd/csrc/act_plan.h)
// on the CPU.  tests/test_act_band_cpu.py builds this with the address and undefined-behaviour sanitizers and runs it.  For every stack, as
// planned and with the band count / panel width forced as SMARTIES_HIP_GENERIC bit 8192 forces them: the bands cover every output row
// once, their input rows lie inside the image, the layout stays within 160 KB; then the banded first layer is carried out as
// act_conv_band_dev_kernel carries it out -- a band buffer on the heap of exactly the planned size, filled band by band, every output formed
// through the planned offset table and the position's base relative to the band -- and compared, float for float, with the convolution
// summed directly over the whole image in the order of Conv2DLayer::forward (Network/Layers/Layer_Conv2D.h:98-110: channel, filter row,
// filter column).  An index outside the band buffer is the sanitizer's to report.
#include "../../smarties_amd/csrc/act_plan.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace hl;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <typename T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }
static unsigned lcg = 12345u;
static float rnd() { lcg = lcg * 1664525u + 1013904223u; return (float)((lcg >> 8) & 0xffff) / 32768.f - 1.f; }

struct Geo { int iw, ih, ic, kn, fs, st; };      // (input_width, input_height, input_features, kernels_num, filters_size, stride)
struct Stack { const char* name; std::vector<Geo> L; int extras; };

static ActConvArgs convArgs(const Stack& s) {
  ActConvArgs a{};
  a.nL = (int)s.L.size(); a.recurrent = 0;
  long long ind = 0;
  for (int l = 0; l < a.nL; ++l) {
    const Geo& g = s.L[l];
    ActConvLayer& L = a.L[l];
    L.InC = g.ic; L.InY = g.ih; L.InX = g.iw; L.KnC = g.kn; L.KnY = L.KnX = g.fs; L.S = g.st;
    L.OpY = (g.ih - g.fs) / g.st + 1; L.OpX = (g.iw - g.fs) / g.st + 1;
    L.K = g.ic * g.fs * g.fs; L.P = L.OpY * L.OpX;
    L.indW = ind; ind += (long long)L.KnC * L.K; L.indB = ind; ind += (long long)L.KnC * L.P;
  }
  a.dIn = s.L[0].ic * s.L[0].ih * s.L[0].iw + s.extras; a.dS = a.dIn;
  return a;
}

// the first layer in bands on a random image against the direct sum
static void emulate(const char* name, const ActConvArgs& a) {
  const ActConvLayer& L = a.L[0];
  const size_t img = (size_t)L.InC * L.InY * L.InX, nW = (size_t)L.KnC * L.K, bandFloats = (size_t)L.InC * a.bandRows * L.InX;
  auto image = exact<float>(img); auto filt = exact<float>(nW);
  for (size_t i = 0; i < img; ++i) image[i] = rnd();
  for (size_t i = 0; i < nW; ++i) filt[i] = rnd();
  CHECK((size_t)(a.bufOff[0] - a.bandOff) >= bandFloats && (size_t)(a.bufOff[0] - a.bandOff) < bandFloats + 4, "%s: the band buffer is not what the layout leaves room for", name);
  auto tab = exact<int>((size_t)L.K);      // the table acTables<true> builds: channel pitch bandRows InX
  const int fsz = L.KnY * L.KnX;
  for (int k = 0; k < L.K; ++k) { const int ic = k / fsz, f = k - ic * fsz, fy = f / L.KnX, fx = f - fy * L.KnX; tab[k] = (ic * a.bandRows + fy) * L.InX + fx; }
  auto band = exact<float>(bandFloats);
  auto seen = exact<int>((size_t)L.P);
  for (int p = 0; p < L.P; ++p) seen[p] = 0;
  for (int b = 0; b < a.nb; ++b) {
    const ActBand d = act_conv_band(a, b);
    for (size_t i = 0; i < bandFloats; ++i) band[i] = 1e30f;      // (a value of the band before: a wrong sum if read)
    for (int ic = 0; ic < L.InC; ++ic)
      for (int e = 0; e < d.rows * L.InX; ++e) band[(size_t)ic * a.bandRows * L.InX + e] = image[((size_t)ic * L.InY + d.iy0) * L.InX + e];
    for (int pos = d.oy0 * L.OpX; pos < d.oy1 * L.OpX; ++pos) {
      const int oy = pos / L.OpX, ox = pos - oy * L.OpX, pb = ((oy - d.oy0) * L.InX + ox) * L.S;
      ++seen[pos];
      for (int c = 0; c < L.KnC; ++c) {
        float viaBand = 0.f, direct = 0.f;
        for (int k = 0; k < L.K; ++k) viaBand += filt[(size_t)c * L.K + k] * band[tab[k] + pb];
        for (int ic = 0; ic < L.InC; ++ic) for (int fy = 0; fy < L.KnY; ++fy) for (int fx = 0; fx < L.KnX; ++fx)
          direct += filt[(((size_t)c * L.InC + ic) * L.KnY + fy) * L.KnX + fx] * image[((size_t)ic * L.InY + oy * L.S + fy) * L.InX + ox * L.S + fx];
        CHECK(viaBand == direct, "%s: band %d channel %d position %d: %g through the band, %g directly", name, b, c, pos, viaBand, direct);
      }
    }
  }
  for (int p = 0; p < L.P; ++p) CHECK(seen[p] == 1, "%s: position %d formed %d times", name, p, seen[p]);
}

static void checkBands(const Stack& s, int force, int wantNb) {
  ActConvArgs a = convArgs(s);
  char name[96]; std::snprintf(name, sizeof name, "%s%s", s.name, force ? " (forced)" : "");
  const bool ok = act_conv_band_plan(&a, force);
  CHECK(ok, "%s: refused", name);
  if (!ok) return;
  const ActConvLayer& L = a.L[0];
  CHECK(a.ldsBytes <= 160 * 1024, "%s: %zu bytes of LDS", name, a.ldsBytes);
  CHECK(a.nb >= 1 && a.nb <= L.OpY && a.bandR == (L.OpY + a.nb - 1) / a.nb, "%s: %d bands of %d rows for %d output rows", name, a.nb, a.bandR, L.OpY);
  if (wantNb) CHECK(a.nb == wantNb, "%s: %d bands, expected %d", name, a.nb, wantNb);
  if (force) CHECK(a.nb == std::min(force, L.OpY) || (a.nb < force && (a.nb - 1) * a.bandR < L.OpY), "%s: %d bands under the switch", name, a.nb);
  auto rowSeen = exact<int>((size_t)L.OpY);
  for (int y = 0; y < L.OpY; ++y) rowSeen[y] = 0;
  for (int b = 0; b < a.nb; ++b) {
    const ActBand d = act_conv_band(a, b);
    CHECK(d.oy0 < d.oy1 && d.oy1 <= L.OpY, "%s: band %d covers [%d, %d)", name, b, d.oy0, d.oy1);
    CHECK(d.iy0 >= 0 && d.rows >= 1 && d.rows <= a.bandRows && d.iy0 + d.rows <= L.InY, "%s: band %d reads rows [%d, %d) of %d (buffer of %d)", name, b, d.iy0, d.iy0 + d.rows, L.InY, a.bandRows);
    for (int y = d.oy0; y < d.oy1 && y < L.OpY; ++y) ++rowSeen[y];
    if (a.bandVec) CHECK((d.iy0 * L.InX) % 4 == 0 && (d.rows * L.InX) % 4 == 0 && (L.InY * L.InX) % 4 == 0 && (a.bandRows * L.InX) % 4 == 0 && a.dS % 4 == 0, "%s: band %d: 16-byte loads on a slice that is no multiple of 4 floats", name, b);
  }
  for (int y = 0; y < L.OpY; ++y) CHECK(rowSeen[y] == 1, "%s: output row %d in %d bands", name, y, rowSeen[y]);
  emulate(name, a);
}

static ActRowsArgs rowsArgs(int nIn, int hidden) {
  ActRowsArgs a{};
  a.dS = a.dIn = nIn; a.nL = 1; a.nDense = 7; a.nSig = 2; a.nOut = 9; a.ldWo = 8;
  a.L[0] = ActLayer{nIn, hidden, (hidden + 3) & ~3, 0, 1, std::min(nIn, hidden), 0, 0, 0, 0};
  return a;
}
static void checkPanels(int nIn, int force) {
  ActRowsArgs a = rowsArgs(nIn, 512);
  const bool ok = act_rows_panel_plan(&a, force);
  CHECK(ok, "panels of a row of %d%s: refused", nIn, force ? " (forced)" : "");
  if (!ok) return;
  CHECK(a.pn >= 32 && a.pn % 32 == 0 && a.pn <= 1024 && (!force || a.pn == force), "row of %d: panels of %d", nIn, a.pn);
  CHECK(a.ldsBytes <= 160 * 1024 && a.ldsBytes == (size_t)(a.panOff + 16 * (a.pn + 4)) * sizeof(float) && a.panOff == 16 * (a.ld + a.ldO), "row of %d: layout", nIn);
  CHECK(a.ld >= 512 + 4 && a.ld % 32 == 4, "row of %d: activations' pitch %d", nIn, a.ld);
  // the kernel's walk: k0 = 0, pn, 2 pn, ..; every panel but the last is whole, the last ends the row
  auto cover = exact<int>((size_t)nIn);
  for (int k = 0; k < nIn; ++k) cover[k] = 0;
  int tails = 0;
  for (int k0 = 0; k0 < a.dIn; k0 += a.pn) {
    const int w = std::min(a.pn, a.dIn - k0);
    CHECK(k0 % 32 == 0, "row of %d: a panel starts at %d", nIn, k0);
    if (w != a.pn) ++tails;
    for (int c = 0; c < w; ++c) ++cover[k0 + c];
  }
  CHECK(tails <= 1, "row of %d: %d tails", nIn, tails);
  for (int k = 0; k < nIn; ++k) CHECK(cover[k] == 1, "row of %d: column %d staged %d times", nIn, k, cover[k]);
}

int main() {
  const Stack nature{"nature", {{84, 84, 4, 32, 8, 4}, {20, 20, 32, 64, 4, 2}, {9, 9, 64, 64, 3, 1}}, 0};
  const Stack stacks[] = {
    nature,
    {"image-176K", {{210, 210, 1, 2, 10, 8}}, 0},
    {"RACER_atari", {{84, 84, 4, 8, 8, 4}, {20, 20, 8, 16, 6, 2}, {8, 8, 16, 32, 4, 1}, {5, 5, 32, 64, 3, 1}}, 0},
    {"9x7x3", {{9, 7, 3, 5, 3, 1}}, 0},
    {"10x10x8", {{10, 10, 8, 16, 6, 2}}, 0},
    {"12x12x4", {{12, 12, 4, 8, 3, 1}}, 5},
  };
  for (const Stack& s : stacks) {
    checkBands(s, 0, &s == &stacks[0] ? 2 : 0);
    checkBands(s, 3, 0);
  }
  {
    ActConvArgs a = convArgs(nature);
    CHECK(act_conv_band_plan(&a) && a.nb == 2 && a.bandR == 10 && a.bandRows == 44 && a.bandVec == 1, "nature: %d bands of %d rows, %d input rows", a.nb, a.bandR, a.bandRows);
    CHECK((size_t)(a.bufOff[0] - a.bandOff) * sizeof(float) == 59136, "nature: a band buffer of %zu bytes", (size_t)(a.bufOff[0] - a.bandOff) * sizeof(float));
    CHECK(!act_conv_wide_plan(&a), "nature: the whole image fits");
    const Stack map{"map-162K", {{38, 38, 1, 32, 3, 1}, {36, 36, 32, 2, 4, 4}}, 0};
    a = convArgs(map);
    CHECK(!act_conv_band_plan(&a) && !act_conv_band_plan(&a, 3), "map-162K: served");
    const Stack wide{"feature row of 8200", {{18, 10, 1, 64, 3, 1}}, 8};      // 8 extras + 64 x 8 x 16
    a = convArgs(wide);
    CHECK(!act_conv_band_plan(&a) && !act_conv_wide_plan(&a), "a feature row of 8200: served");
  }
  for (int nIn : {189, 2048, 2049, 2357, 3136, 8192}) { checkPanels(nIn, 0); checkPanels(nIn, 64); }
  {
    ActRowsArgs a = rowsArgs(8193, 512);
    CHECK(!act_rows_panel_plan(&a) && !act_rows_panel_plan(&a, 64), "an input row of 8193: served");
    a = rowsArgs(3136, 2049);
    CHECK(!act_rows_panel_plan(&a), "a layer of 2049: served");
    a = rowsArgs(3136, 2048);
    CHECK(act_rows_panel_plan(&a) && a.ng == 8 && a.ldsBytes <= 160 * 1024, "a layer of 2048 behind a row of 3136: refused");
  }
  if (failures) { std::printf("act_plan_check: %d failures\n", failures); return 1; }
  std::printf("act_plan_check: ok\n");
  return 0;
}
