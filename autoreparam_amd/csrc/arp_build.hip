// What a model id is on the host: the builders that turn a dataset into a handle's sufficient statistics and device
// tables, and the family table (host_common.h: Family) that names each model's builder, launcher table and selection policy.
#include <math.h>
#include <string.h>
#include <algorithm>
#include "host_common.h"

namespace arp {

static const double kHalfLog2Pi = 0.9189385332046727;

static int upload_tables(arp_model* m);

static int build_radon(arp_model* m, const arp_dataset* d) {
  m->args = &m->radon;
  const int J = d->n_groups, N = d->n_obs;
  if (!d->group_host || !d->u_host || !d->x_host || !d->y_host || J <= 0 || N <= 0) {
    set_error("radon: group/u/x/y and n_groups/n_obs are required");
    return 1;
  }
  std::vector<double> n(J, 0.0), sx(J, 0.0), sy(J, 0.0);
  double sxy = 0, sxx = 0, syy = 0;
  for (int i = 0; i < N; ++i) {
    int j = d->group_host[i];
    double x = d->x_host[i], y = d->y_host[i];
    sxy += x * y; sxx += x * x; syy += y * y;
    // tf.one_hot gives an all-zero row for an out-of-range county: such an
    // observation sees no county effect and only informs b2 (models.py:834-836)
    if (j < 0 || j >= J) continue;
    n[j] += 1; sx[j] += x; sy[j] += y;
  }
  m->D = 3 + J;
  m->n_groups = J;
  m->host_tables.resize(4 * (size_t)J);
  for (int j = 0; j < J; ++j) {
    m->host_tables[j] = (float)n[j];
    m->host_tables[J + j] = (float)sx[j];
    m->host_tables[2 * J + j] = (float)sy[j];
    m->host_tables[3 * J + j] = d->u_host[j];
  }
  if (upload_tables(m)) return 1;
  m->radon.n = m->dev_tables;
  m->radon.sx = m->dev_tables + J;
  m->radon.sy = m->dev_tables + 2 * J;
  m->radon.u = m->dev_tables + 3 * J;
  m->radon.sxy = (float)sxy;
  m->radon.sxx = (float)sxx;
  double sy_tot = 0, suy_tot = 0;
  for (int j = 0; j < J; ++j) { sy_tot += sy[j]; suy_tot += (double)d->u_host[j] * sy[j]; }
  m->radon.sy_tot = (float)sy_tot;
  m->radon.suy_tot = (float)suy_tot;
  m->radon.J = J;
  // every Normal has unit scale under every (a,b): const = -(3+J+N) 0.5 log 2pi - 0.5 Syy
  m->const_base = -(3.0 + J + N) * kHalfLog2Pi - 0.5 * syy;
  return 0;
}

static int upload_tables(arp_model* m) {
  if (m->host_only) {
    m->dev_tables = (float*)malloc(std::max<size_t>(1, m->host_tables.size()) * sizeof(float));
    if (!m->dev_tables) { set_error("upload_tables: out of memory"); return 1; }
    memcpy(m->dev_tables, m->host_tables.data(), m->host_tables.size() * sizeof(float));
    return 0;
  }
  ARP_HIP_OK(hipMalloc(&m->dev_tables, m->host_tables.size() * sizeof(float)));
  ARP_HIP_OK(hipMemcpy(m->dev_tables, m->host_tables.data(), m->host_tables.size() * sizeof(float),
                       hipMemcpyHostToDevice));
  return 0;
}

// reference models.py:131-147: y_host = effects, u_host = stddevs
static int build_schools(arp_model* m, const arp_dataset* d) {
  m->args = &m->schools;
  if (!d->y_host || !d->u_host) { set_error("8schools: y (effects) and u (stddevs) are required"); return 1; }
  m->D = 10; m->n_groups = 8;
  m->host_tables.assign(d->y_host, d->y_host + 8);
  m->host_tables.insert(m->host_tables.end(), d->u_host, d->u_host + 8);
  if (upload_tables(m)) return 1;
  m->schools.y = m->dev_tables;
  m->schools.sigma = m->dev_tables + 8;
  double c = -18.0 * kHalfLog2Pi;
  for (int k = 0; k < 8; ++k) c -= log((double)d->u_host[k]);
  m->const_base = c;
  m->top_scale = {{0, log(5.0)}, {1, log(5.0)}};
  return 0;
}

// reference models.py:967-989: group = 1-based state fed to tf.one_hot(., S); x = female, x2 = black
static int build_election(arp_model* m, const arp_dataset* d) {
  m->args = &m->election;
  const int S = d->n_groups, N = d->n_obs;
  if (!d->group_host || !d->x_host || !d->x2_host || !d->y_host || S <= 0 || N <= 0) {
    set_error("election: group/x(female)/x2(black)/y and n_groups/n_obs are required");
    return 1;
  }
  m->D = S + 4; m->n_groups = S + 1;
  std::vector<double> cn((size_t)(S + 1) * 4, 0.0), cy((size_t)(S + 1) * 4, 0.0);
  for (int i = 0; i < N; ++i) {
    int t = d->group_host[i];
    if (t < 0 || t >= S) t = S;  // all-zero one-hot row: no state effect
    int c = (d->x_host[i] != 0.0f ? 1 : 0) + (d->x2_host[i] != 0.0f ? 2 : 0);
    if ((d->x_host[i] != 0.0f && d->x_host[i] != 1.0f) || (d->x2_host[i] != 0.0f && d->x2_host[i] != 1.0f)) {
      set_error("election: female/black must be 0/1 indicators for the cell collapse");
      return 1;
    }
    cn[(size_t)t * 4 + c] += 1.0;
    cy[(size_t)t * 4 + c] += d->y_host[i];
  }
  m->host_tables.resize(cn.size() * 2);
  for (size_t i = 0; i < cn.size(); ++i) { m->host_tables[i] = (float)cn[i]; m->host_tables[cn.size() + i] = (float)cy[i]; }
  if (upload_tables(m)) return 1;
  m->election.cell_n = m->dev_tables;
  m->election.cell_y = m->dev_tables + cn.size();
  m->election.S = S;
  m->const_base = -(4.0 + S) * kHalfLog2Pi;
  m->top_scale = {{0, log(100.0)}, {1, log(10.0)}, {2 + S, log(100.0)}, {3 + S, log(100.0)}};
  return 0;
}

// reference models.py:763-806 (radon_stddvs): same inputs as radon; every county keeps all six
// second-order sufficient statistics because its observation scale is a latent
static int build_radon_sd(arp_model* m, const arp_dataset* d) {
  m->args = &m->radon_sd;
  const int J = d->n_groups, N = d->n_obs;
  if (!d->group_host || !d->u_host || !d->x_host || !d->y_host || J <= 0 || N <= 0) {
    set_error("radon_stddvs: group/u/x/y and n_groups/n_obs are required");
    return 1;
  }
  std::vector<double> st(6 * (size_t)J, 0.0);
  for (int i = 0; i < N; ++i) {
    int j = d->group_host[i];
    if (j < 0 || j >= J) {   // a zero one-hot row would give the observation a zero scale (models.py:785-786)
      set_error("radon_stddvs: county index out of range");
      return 1;
    }
    double x = d->x_host[i], y = d->y_host[i];
    st[j] += 1; st[J + j] += x; st[2 * J + j] += y; st[3 * J + j] += x * x; st[4 * J + j] += x * y; st[5 * J + j] += y * y;
  }
  m->D = 3 + 2 * J; m->n_groups = J;
  m->host_tables.resize(7 * (size_t)J);
  for (size_t k = 0; k < 6 * (size_t)J; ++k) m->host_tables[k] = (float)st[k];
  for (int j = 0; j < J; ++j) m->host_tables[6 * (size_t)J + j] = d->u_host[j];
  if (upload_tables(m)) return 1;
  float* t = m->dev_tables;
  m->radon_sd.n = t; m->radon_sd.sx = t + J; m->radon_sd.sy = t + 2 * J; m->radon_sd.sxx = t + 3 * J;
  m->radon_sd.sxy = t + 4 * J; m->radon_sd.syy = t + 5 * J; m->radon_sd.u = t + 6 * J;
  m->radon_sd.J = J;
  m->const_base = -(3.0 + 2.0 * J + N) * kHalfLog2Pi;
  return 0;
}

// reference models.py:860-904: X = [N][F] design matrix (intercept, standardised
// numerics, one-hot blocks), y = 0/1 outcomes
static int build_german(arp_model* m, const arp_dataset* d) {
  m->args = &m->german;
  const int N = d->n_obs, F = d->n_features;
  if (!d->X_host || !d->y_host || N <= 0 || F <= 0 || F > kGermanCols) {
    set_error("german_credit: X, y, n_obs and 0 < n_features <= 64 are required");
    return 1;
  }
  m->D = 1 + 2 * F; m->n_groups = F;
  // [N][64] rows + outcomes (the 8- and 16-lane likelihoods), then the image the matrix-core likelihood copies
  // into LDS with LDS-DMA (german_image.h, "tile image"): per 128 observations the rows with their 16-byte chunks
  // XOR-permuted, and one piece of outcomes
  const size_t plain = ((size_t)N * kGermanCols + N + 255) & ~(size_t)255;
  const int nt = (N + kGermanTileRows - 1) / kGermanTileRows;
  m->host_tables.assign(plain + (size_t)nt * kGermanImgTile, 0.0f);
  for (int n = 0; n < N; ++n)
    for (int f = 0; f < F; ++f) m->host_tables[(size_t)n * kGermanCols + f] = d->X_host[(size_t)n * F + f];
  for (int n = 0; n < N; ++n) m->host_tables[(size_t)N * kGermanCols + n] = d->y_host[n];
  for (int t = 0; t < nt; ++t) {
    float* img = m->host_tables.data() + plain + (size_t)t * kGermanImgTile;
    for (int r = 0; r < kGermanTileRows; ++r) {
      const int n = t * kGermanTileRows + r;
      if (n >= N) break;
      for (int f = 0; f < F; ++f) img[german_x_word(r, f)] = d->X_host[(size_t)n * F + f];
      img[german_y_word(r)] = d->y_host[n];
    }
  }
  // the bf16 x 3 image (german_image.h): usable when at most 8 columns are not exact in ONE bf16 piece
  const size_t f32_floats = m->host_tables.size();
  std::vector<int> split;
  for (int f = 0; f < F; ++f) {
    bool exact = true;
    for (int n = 0; n < N && exact; ++n) {
      uint32_t h, mm_, l;
      bf3_split(d->X_host[(size_t)n * F + f], h, mm_, l);
      exact = mm_ == 0u && l == 0u;
    }
    if (!exact) split.push_back(f);
  }
  const bool bf3 = (int)split.size() <= kBf3MaxSplit;
  const int ntb = (N + kBf3Rows - 1) / kBf3Rows;
  for (int q = 0; q < kBf3MaxSplit; ++q) m->german.sidx[q] = bf3 && q < (int)split.size() ? split[q] : -1;
  if (bf3) {
    m->host_tables.resize(f32_floats + (size_t)ntb * kBf3ImgTile, 0.0f);
    auto put = [](unsigned char* img, size_t byte_off, uint32_t bits) {      // the bf16 = high half of the f32 pattern
      img[byte_off] = (unsigned char)(bits >> 16); img[byte_off + 1] = (unsigned char)(bits >> 24);
    };
    for (int t = 0; t < ntb; ++t) {
      unsigned char* img = reinterpret_cast<unsigned char*>(m->host_tables.data() + f32_floats + (size_t)t * kBf3ImgTile);
      for (int r = 0; r < kBf3Rows; ++r) {
        const int n = t * kBf3Rows + r;
        if (n >= N) break;
        const Bf3Frag frag = bf3_frag(r);   // where observation r sits in a backward fragment
        for (int f = 0; f < F; ++f) {
          uint32_t h, mm_, l;
          bf3_split(d->X_host[(size_t)n * F + f], h, mm_, l);
          put(img, bf3_xhf_byte(r, f), h);
          put(img, bf3_xhb_byte(frag, f), h);
        }
        for (int q = 0; q < (int)split.size(); ++q) {
          uint32_t h, mm_, l;
          bf3_split(d->X_host[(size_t)n * F + split[q]], h, mm_, l);
          put(img, bf3_xaf_byte(r, 0, q), mm_);       // [xm | xm | xl | 0]
          put(img, bf3_xaf_byte(r, 1, q), mm_);
          put(img, bf3_xaf_byte(r, 2, q), l);
          put(img, bf3_xab_byte(frag, q), mm_);       // output rows q (xm) and 8 + q (xl)
          put(img, bf3_xab_byte(frag, 8 + q), l);
        }
        reinterpret_cast<float*>(img + kBf3Y)[r] = d->y_host[n];
      }
    }
  }
  if (upload_tables(m)) return 1;
  m->german.X = m->dev_tables;
  m->german.y = m->dev_tables + (size_t)N * kGermanCols;
  m->german.Xt = m->dev_tables + plain;
  m->german.Xb = bf3 ? m->dev_tables + f32_floats : nullptr;
  m->german.N = N; m->german.F = F;
  m->const_base = -(1.0 + 2.0 * F) * kHalfLog2Pi;
  m->top_scale = {{0, log(10.0)}};
  return 0;
}

// reference models.py:1011-1046: group = pair, group2 = grade, group3 = grade_pair (all 1-based, fed to
// tf.one_hot as they are), x = treatment, y = scores.  Observations collapse to (pair, treatment) cells.
static int build_electric(arp_model* m, const arp_dataset* d) {
  m->args = &m->electric;
  const int P = d->n_groups, N = d->n_obs, G = d->n_features;
  if (!d->group_host || !d->group2_host || !d->group3_host || !d->x_host || !d->y_host || P <= 0 || N <= 0) {
    set_error("electric: group(pair)/group2(grade)/group3(grade_pair)/x(treatment)/y and n_groups/n_obs are required");
    return 1;
  }
  if (G != kElG) { set_error("electric: n_features (n_grade = n_grade_pair) must be 4"); return 1; }
  const int R = P + 1;   // group P: observations whose pair index falls on the all-zero one-hot row
  std::vector<double> n(2 * (size_t)R, 0.0), sy(2 * (size_t)R, 0.0), syy(2 * (size_t)R, 0.0);
  std::vector<int> grade(R, -1);
  for (int i = 0; i < N; ++i) {
    int j = d->group_host[i];
    if (j < 0 || j >= P) j = P;
    int g = d->group2_host[i];
    if (g < 0 || g >= G) g = G;   // zero row: b = 0, scale exp(0)
    const float t = d->x_host[i];
    if (t != 0.0f && t != 1.0f) { set_error("electric: treatment must be a 0/1 indicator for the cell collapse"); return 1; }
    if (grade[j] >= 0 && grade[j] != g) {
      set_error("electric: the observations of one pair must share a grade for the cell collapse");
      return 1;
    }
    grade[j] = g;
    const size_t c = (size_t)(t != 0.0f) * R + j;
    const double y = d->y_host[i];
    n[c] += 1; sy[c] += y; syy[c] += y * y;
  }
  m->D = 3 * G + P; m->n_groups = R;
  m->host_tables.assign(13 * (size_t)R, 0.0f);
  float* T = m->host_tables.data();
  for (int j = 0; j < R; ++j) {
    if (j < P) {
      const int k = d->group3_host[j];
      if (k >= 0 && k < G) T[(size_t)k * R + j] = 100.0f;
    }
    if (grade[j] >= 0 && grade[j] < G) T[(size_t)(4 + grade[j]) * R + j] = 1.0f;
    double ss = 0;
    for (int t = 0; t < 2; ++t) {
      const size_t c = (size_t)t * R + j;
      const double mean = n[c] > 0 ? sy[c] / n[c] : 0.0;
      T[(size_t)(8 + 2 * t) * R + j] = (float)n[c];
      T[(size_t)(9 + 2 * t) * R + j] = (float)mean;
      ss += syy[c] - n[c] * mean * mean;
    }
    T[(size_t)12 * R + j] = (float)(ss > 0 ? ss : 0.0);
  }
  if (upload_tables(m)) return 1;
  float* t = m->dev_tables;
  m->electric.wm = t; m->electric.og = t + 4 * (size_t)R;
  m->electric.n0 = t + 8 * (size_t)R; m->electric.y0 = t + 9 * (size_t)R;
  m->electric.n1 = t + 10 * (size_t)R; m->electric.y1 = t + 11 * (size_t)R;
  m->electric.ss = t + 12 * (size_t)R;
  m->electric.P = P;
  m->const_base = -(double)(m->D + N) * kHalfLog2Pi;
  for (int k = 0; k < G; ++k) m->top_scale.push_back({2 * G + P + k, log(100.0)});
  return 0;
}

// reference models.py:1069-1141: x = regressor (years), y = series, n_obs = T
static int build_time_series(arp_model* m, const arp_dataset* d) {
  m->args = &m->time_series;
  const int T = d->n_obs;
  if (!d->x_host || !d->y_host || T <= 0) { set_error("time_series: x, y and n_obs are required"); return 1; }
  // the block scan splits the T steps over the lanes of a chain in blocks of ceil(T / K) (the last lanes padded); the
  // instantiations of inst_time_series.hip are those of the reference's T = 60
  if (T != kTsSteps) { set_error("time_series: n_obs must be 60 (add TimeSeriesLane<K, 2 ceil(T / K)> to inst_time_series.hip for another length)"); return 1; }
  m->D = 3 + 2 * T; m->n_groups = 2 * T;
  m->host_tables.assign(d->x_host, d->x_host + T);
  m->host_tables.insert(m->host_tables.end(), d->y_host, d->y_host + T);
  if (upload_tables(m)) return 1;
  m->time_series.x = m->dev_tables;
  m->time_series.y = m->dev_tables + T;
  m->time_series.T = T;
  m->const_base = -(double)(m->D + T) * kHalfLog2Pi - T * log(0.12);
  return 0;
}

// reference models.py:671-696: no data
static int build_funnel(arp_model* m, const arp_dataset*) {
  m->args = &m->funnel;
  m->D = 2; m->n_groups = 1; m->const_base = -2.0 * kHalfLog2Pi; m->top_scale = {{0, log(3.0)}};
  return 0;
}

// One row per ARP_MODEL_*, in the order of the ids.  Default lanes per chain (arp_api.hip: pick): the fewest that put
// fill_lanes lanes on the device -- two waves on every SIMD of the 256 CUs (256 x 4 x 2 x 64 = 131072) unless the family
// measured better with one:
// radon: a wider split costs more replicated work than a second wave per SIMD returns (bench.py --chains 8192: 1.21e10
// leapfrog-steps/s at 8 lanes per chain, 1.07e10 at 16), so one wave per SIMD is enough;
// time_series likewise: 4 lanes per chain (one wave per SIMD at 16 384 chains) beat 8 and 16 in every form wherever they
// fill the SIMDs once (round 3 sweep, profiles/r03_time_series_sweep.txt); a lane owns whole time steps (unit = 2);
// german credit: the 4-lane instantiation runs its likelihood on the matrix cores and beats the wider ones at every chain
// count (per workgroup 4x the 8-lane and 17x the 16-lane rate), and is the VI kernel's; its lanes tile the padded 64
// columns whatever F is (not exact).  `ops` is the log-normal prior's table: arp_api.hip: lane_ops swaps in the variant's.
static constexpr Family kFamilies[] = {
    // id, builder, launcher table, exact, unit, fill_lanes, default_lanes, vi_lanes
    {ARP_MODEL_EIGHT_SCHOOLS, build_schools, schools_ops, true, 1, 131072, 0, 0},
    {ARP_MODEL_RADON, build_radon, radon_ops, true, 1, 65536, 0, 0},
    {ARP_MODEL_GERMAN_CREDIT, build_german, german_ops, false, 1, 131072, 4, 4},
    {ARP_MODEL_ELECTION, build_election, election_ops, true, 1, 131072, 0, 0},
    {ARP_MODEL_RADON_STDDVS, build_radon_sd, radon_sd_ops, true, 1, 131072, 0, 0},
    {ARP_MODEL_NEALS_FUNNEL, build_funnel, funnel_ops, true, 1, 131072, 0, 0},
    {ARP_MODEL_ELECTRIC, build_electric, electric_ops, true, 1, 131072, 0, 0},
    {ARP_MODEL_TIME_SERIES, build_time_series, time_series_ops, true, 2, 65536, 0, 0},
};
constexpr int kNumFamilies = sizeof(kFamilies) / sizeof(kFamilies[0]);
constexpr bool families_in_id_order() {
  for (int i = 0; i < kNumFamilies; ++i) if (kFamilies[i].model != i) return false;
  return true;
}
static_assert(families_in_id_order(), "kFamilies is indexed by ARP_MODEL_*");

const Family* family_of(int model) { return model >= 0 && model < kNumFamilies ? &kFamilies[model] : nullptr; }

}  // namespace arp
