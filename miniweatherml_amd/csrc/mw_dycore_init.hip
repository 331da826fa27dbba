// =====================================================================================================
// mw_dycore_init.hip -- initial data (input construction, :1197-1683, :1687-1887) and the temperature perturbations.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#include <cmath>
#include <random>

namespace mw {

// -----------------------------------------------------------------------------------------------------
// Initial data (input construction, :1197-1683, :1687-1887).  Column profiles are built on the host
// (further down); the per-cell quadrature + convert_dynamics_to_coupler (:1656) runs here.
// -----------------------------------------------------------------------------------------------------
struct InitP {
  int init_data, ord;
  long long i_beg, j_beg;
  double xlen, ylen, cp_d, p0;
  const double *hyDensGLL, *hyDensThetaGLL, *hyDensVapGLL;     // supercell: (nz,5) device
  const double *bheights; int nbx, nby, cells_per_building, buildings_pad, nblocks_x, nblocks_y;   // city
  long long nx_glob, ny_glob;
};

__device__ __forceinline__ void d_hydro_const_theta(double z, double grav, double C0, double cp, double p0, double gamma,
                                                    double rd, double &r, double &t) {     // :1108-1117
#pragma clang fp contract(off)
  const double theta0 = 300., exner0 = 1.;
  t = theta0;
  double exner = exner0 - grav * z / (cp * theta0);
  double pr = p0 * pow_ref(exner, (cp / rd));
  double rt = pow_ref((pr / C0), (1.0 / gamma));
  r = rt / t;
}
__device__ __forceinline__ double d_sample_ellipse_cosine(double amp, double x, double y, double z, double x0, double y0,
                                                          double z0, double xrad, double yrad, double zrad) {   // :1121-1134
#pragma clang fp contract(off)
  double dist = sqrt(((x - x0) / xrad) * ((x - x0) / xrad) + ((y - y0) / yrad) * ((y - y0) / yrad) +
                     ((z - z0) / zrad) * ((z - z0) / zrad)) * M_PI / 2.;
  if (dist <= M_PI / 2.) return amp * pow_ref(cos_ref(dist), 2.0);
  return 0.;
}

__constant__ double c_gll5_pts[5] = {-0.50000000000000000000000000000000000000, -0.32732683535398857189914622812342917778,
                                     0.00000000000000000000000000000000000000, 0.32732683535398857189914622812342917778,
                                     0.50000000000000000000000000000000000000};      // TransformMatrices.h:650-656
__constant__ double c_gll5_wts[5] = {0.050000000000000000000000000000000000000, 0.27222222222222222222222222222222222222,
                                     0.35555555555555555555555555555555555556, 0.27222222222222222222222222222222222222,
                                     0.050000000000000000000000000000000000000};     // :659-665
__constant__ double c_gll3_pts[3] = {-0.50000000000000000000000000000000000000, 0.00000000000000000000000000000000000000,
                                     0.50000000000000000000000000000000000000};      // TransformMatrices.h:83-88 (MW_ORD = 3)
__constant__ double c_gll3_wts[3] = {0.16666666666666666666666666666666666667, 0.66666666666666666666666666666666666667,
                                     0.16666666666666666666666666666666666667};      // :90-95
__constant__ double c_gll9_pts[9] = {-0.50000000000000000000000000000000000000, -0.44987899770573007865617262220916897903,
                                     -0.33859313975536887672294271354567122536, -0.18155873191308907935537603435432960651,
                                     0.00000000000000000000000000000000000000, 0.18155873191308907935537603435432960651,
                                     0.33859313975536887672294271354567122536, 0.44987899770573007865617262220916897903,
                                     0.50000000000000000000000000000000000000};      // :4113-4124
__constant__ double c_gll9_wts[9] = {0.013888888888888888888888888888888888889, 0.082747680780402762523169860014604152919,
                                     0.13726935625008086764035280928968636297, 0.17321425548652317255756576606985914397,
                                     0.18575963718820861678004535147392290249, 0.17321425548652317255756576606985914397,
                                     0.13726935625008086764035280928968636297, 0.082747680780402762523169860014604152919,
                                     0.013888888888888888888888888888888888889};     // :4126-4137
__constant__ double c_gll7_pts[7] = MW_GLL7_PTS;                                    // get_gll_points / _weights(SArray<FP,1,7>): mw_weno79.h
__constant__ double c_gll7_wts[7] = MW_GLL7_WTS;
__constant__ double c_gl3_pts[3] = {0.112701665379258311482073460022, 0.500000000000000000000000000000,
                                    0.887298334620741688517926539980};                // :1349-1351
__constant__ double c_gl3_wts[3] = {0.277777777777777777777777777779, 0.444444444444444444444444444444,
                                    0.277777777777777777777777777779};                // :1353-1355

__global__ __launch_bounds__(256) void k_init_cells(DyP p, InitP q, CouplerPtrs c, double *__restrict__ imm) {
#pragma clang fp contract(off)
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int k = blockIdx.y;
  int NXI = p.nx * p.nens;
  if (t >= (long long)p.ny * NXI) return;
  int j = (int)(t / NXI), ie = (int)(t - (long long)j * NXI);
  int i = ie / p.nens, e = ie - i * p.nens;
  long long ci = ((long long)k * p.ny + j) * NXI + ie;
  double sR = 0, sU = 0, sV = 0, sW = 0, sT = 0, sWV = 0;
  const double dx = p.dx, dy = p.dy, dz = p.dz;
  if (q.init_data == MW_DATA_SUPERCELL) {                     // :1843-1886  (ord GLL points per direction)
    const int no = q.ord;
    const double *gp = (no == 3) ? c_gll3_pts : (no == 7) ? c_gll7_pts : (no == 9) ? c_gll9_pts : c_gll5_pts;
    const double *gw = (no == 3) ? c_gll3_wts : (no == 7) ? c_gll7_wts : (no == 9) ? c_gll9_wts : c_gll5_wts;
    for (int kk = 0; kk < no; kk++) for (int jj = 0; jj < no; jj++) for (int ii = 0; ii < no; ii++) {
      double zloc = (k + 0.5) * dz + gp[kk] * dz;
      double dens = q.hyDensGLL[k * no + kk];
      double uvel;
      const double zs = 5000, us = 30, uc = 15;
      if (zloc < zs) uvel = us * (zloc / zs) - uc; else uvel = us - uc;
      double vvel = 0, wvel = 0;
      double dens_vap = q.hyDensVapGLL[k * no + kk], dens_theta = q.hyDensThetaGLL[k * no + kk];
      double factor = gw[ii] * gw[jj] * gw[kk];
      sR += (dens - q.hyDensGLL[k * no + kk]) * factor;
      sU += dens * uvel * factor;
      sV += dens * vvel * factor;
      sW += dens * wvel * factor;
      sT += (dens_theta - q.hyDensThetaGLL[k * no + kk]) * factor;
      sWV += dens_vap * factor;
    }
  } else {                                                     // thermal :1361-1392 ; city :1463-1503 ; building :1566-1607
    const int nq = (q.init_data == MW_DATA_THERMAL) ? 3 : 9;
    const double *qp = (q.init_data == MW_DATA_THERMAL) ? c_gl3_pts : c_gll9_pts;
    const double *qw = (q.init_data == MW_DATA_THERMAL) ? c_gl3_wts : c_gll9_wts;
    for (int kk = 0; kk < nq; kk++) for (int jj = 0; jj < nq; jj++) for (int ii = 0; ii < nq; ii++) {
      double x = (i + q.i_beg + 0.5) * dx + (qp[ii] - 0.5) * dx;
      double y = (j + q.j_beg + 0.5) * dy + (qp[jj] - 0.5) * dy;   if (p.sim2d) y = q.ylen / 2;
      double z = (k + 0.5) * dz + (qp[kk] - 0.5) * dz;
      double rho, u, v, w, theta, rho_v, hr, ht;
      if (q.init_data == MW_DATA_THERMAL) {                    // thermal(), :1086-1103
        d_hydro_const_theta(z, p.grav, p.C0, q.cp_d, q.p0, p.gamma, p.R_d, hr, ht);
        double rho_d = hr;
        u = 0.; v = 0.; w = 0.;
        double theta_d = ht + d_sample_ellipse_cosine(2.0, x, y, z, q.xlen / 2, q.ylen / 2, 2000., 2000., 2000., 2000.);
        double p_d = p.C0 * pow_ref(rho_d * theta_d, p.gamma);
        double temp = p_d / rho_d / p.R_d;
        double tc = temp - 273.15;                             // saturation_vapor_pressure, :1137-1140
        double sat_pv = 610.94 * exp_ref(17.625 * tc / (243.04 + tc));
        double sat_rv = sat_pv / p.R_v / temp;
        rho_v = d_sample_ellipse_cosine(0.8, x, y, z, q.xlen / 2, q.ylen / 2, 2000., 2000., 2000., 2000.) * sat_rv;
        double pr = rho_d * p.R_d * temp + rho_v * p.R_v * temp;
        rho = rho_d + rho_v;
        theta = pow_ref(pr / p.C0, 1.0 / p.gamma) / rho;
      } else {
        if (p.enable_gravity) d_hydro_const_theta(z, p.grav, p.C0, q.cp_d, q.p0, p.gamma, p.R_d, hr, ht);
        else { hr = 1.15; ht = 300; }
        rho = hr; u = 20; v = 0; w = 0; theta = ht; rho_v = 0;
      }
      if (p.sim2d) v = 0;
      double wt = qw[ii] * qw[jj] * qw[kk];
      sR += (rho - hr) * wt;
      sU += rho * u * wt;
      sV += rho * v * wt;
      sW += rho * w * wt;
      sT += (rho * theta - hr * ht) * wt;
      sWV += rho_v * wt;
    }
    if (q.init_data == MW_DATA_CITY) {                         // :1504-1514
      int inorm = ((int)q.i_beg + i) / q.cells_per_building - q.buildings_pad;
      int jnorm = ((int)q.j_beg + j) / q.cells_per_building - q.buildings_pad;
      if ((inorm >= 0 && inorm < q.nblocks_x * 3 && inorm % 3 < 2) && (jnorm >= 0 && jnorm < q.nblocks_y * 9 && jnorm % 9 < 8)) {
        if (k <= ceil(q.bheights[(long long)jnorm * q.nbx + inorm] / dz)) imm[ci] = 1;
      }
    } else if (q.init_data == MW_DATA_BUILDING) {              // :1608-1617
      double x0 = 0.3 * q.nx_glob, y0 = 0.5 * q.ny_glob, xr = 0.05 * q.ny_glob, yr = 0.05 * q.ny_glob;
      if (fabs((double)(q.i_beg + i) - x0) <= xr && fabs((double)(q.j_beg + j) - y0) <= yr && k <= 0.2 * p.nz) imm[ci] = 1;
    }
  }
  // convert_dynamics_to_coupler (:1927-1950); all tracers other than water vapour start at zero
  double hyc = p.hyc[k * p.nens + e], hytc = p.hytc[k * p.nens + e];
  double rho = sR + hyc;
  double u = sU / rho, v = sV / rho, w = sW / rho;
  double theta = (sT + hytc) / rho;
  double press = p.C0 * pow_ref(rho * theta, p.gamma);
  double rho_d = rho;
  for (int tr = 0; tr < p.nt; tr++) {
    double val = (tr == p.idWV) ? sWV : 0.0;
    if ((p.mass_mask >> tr) & 1u) rho_d -= val;
    c.tr[tr][ci] = val;
  }
  double temp = press / (rho_d * p.R_d + sWV * p.R_v);
  c.rho_d[ci] = rho_d; c.u[ci] = u; c.v[ci] = v; c.w[ci] = w; c.temp[ci] = temp;
}

// modules::perturb_temperature(thermal=true)   perturb_temperature.h:41-66
__global__ __launch_bounds__(256) void k_perturb_temperature(int nz, int ny, int nx, int nens, long long i_beg, long long j_beg,
                                                             double dx, double dy, double dz, double xlen, double ylen,
                                                             double *__restrict__ temp) {
#pragma clang fp contract(off)
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  long long n = (long long)nz * ny * nx * nens;
  if (t >= n) return;
  long long r = t / nens;
  int i = (int)(r % nx); r /= nx;
  int j = (int)(r % ny); int k = (int)(r / ny);
  double xloc = (i + i_beg + 0.5) * dx, yloc = (j + j_beg + 0.5) * dy, zloc = (k + 0.5) * dz;
  double x0 = xlen / 2, y0 = ylen / 2, z0 = 1500, radx = 10000, rady = 10000, radz = 1500, amp = 5;
  double xn = (xloc - x0) / radx, yn = (yloc - y0) / rady, zn = (zloc - z0) / radz;
  double rad = sqrt(xn * xn + yn * yn + zn * zn);
  if (rad < 1) temp[t] += amp * pow_ref(cos_ref(M_PI * rad / 2), 2.0);
}

// modules::perturb_temperature(random=true)   perturb_temperature.h:25-39: the lowest nz/4 levels get uniform noise in [-1, 1] * 3 K,
// fading linearly with height; every (level, column) draws from its own generator seeded with a globally unique key
// (myrank*nz*nx*ny*nens + k*ncol + i).  yakl::Random is not available (empty submodule): the same key goes through the splitmix64
// finaliser (53 random bits -> [0, 1)), the substitution the surrogate-data sampler uses (mw_output.hip); INTEGRATION.md says so.
__global__ __launch_bounds__(256) void k_perturb_temperature_random(int num_levels, long long ncol, unsigned long long seed,
                                                                    double *__restrict__ temp) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)num_levels * ncol) return;
  const int k = (int)(t / ncol);
  unsigned long long z = seed + (unsigned long long)t + 0x9E3779B97F4A7C15ull;              // t = k*ncol + i
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const double u01 = (double)(z >> 11) * (1.0 / 9007199254740992.0);
  const double rnd = u01 * 2.0 - 1.0;
  const double scaling = (num_levels - (double)k) / num_levels;
  temp[t] += rnd * 3.0 * scaling;                               // (levels are the slowest index: t addresses temp(k, column) directly)
}

} // namespace mw

// ---- init (:1197-1683): host column profiles + device quadrature --------------------------------------
namespace {

double h_supercell_temperature(double z, double z_0, double z_trop, double z_top, double T_0, double T_trop, double T_top) {  // :1144-1153
  if (z <= z_trop) { double lapse = -(T_trop - T_0) / (z_trop - z_0); return T_0 - lapse * (z - z_0); }
  double lapse = -(T_top - T_trop) / (z_top - z_trop);
  return T_trop - lapse * (z - z_trop);
}
double h_supercell_pressure_dry(double z, double z_0, double z_trop, double z_top, double T_0, double T_trop, double T_top,
                                double p_0, double R_d, double grav) {          // :1157-1177
  if (z <= z_trop) {
    double lapse = -(T_trop - T_0) / (z_trop - z_0);
    double T = h_supercell_temperature(z, z_0, z_trop, z_top, T_0, T_trop, T_top);
    return p_0 * pow(T / T_0, grav / (R_d * lapse));
  }
  double lapse = -(T_trop - T_0) / (z_trop - z_0);
  double p_trop = p_0 * pow(T_trop / T_0, grav / (R_d * lapse));
  lapse = -(T_top - T_trop) / (z_top - z_trop);
  if (lapse != 0) {
    double T = h_supercell_temperature(z, z_0, z_trop, z_top, T_0, T_trop, T_top);
    return p_trop * pow(T / T_trop, grav / (R_d * lapse));
  }
  return p_trop * exp(-grav * (z - z_trop) / (R_d * T_trop));
}
double h_supercell_relhum(double z, double, double z_trop) {                    // :1181-1187
  if (z <= z_trop) return 1.0 - 0.75 * pow(z / z_trop, 1.25);
  return 0.25;
}
double h_supercell_sat_mix_dry(double press, double T) { return 380 / (press)*exp(17.27 * (T - 273) / (T - 36)); }   // :1191-1193

void h_hydro_const_theta(double z, double grav, double C0, double cp, double p0, double gamma, double rd, double &r, double &t) {   // :1108-1117
  const double theta0 = 300., exner0 = 1.;
  t = theta0;
  double exner = exner0 - grav * z / (cp * theta0);
  double p = p0 * std::pow(exner, (cp / rd));
  double rt = std::pow((p / C0), (1.0 / gamma));
  r = rt / t;
}

const double h_gll5_pts[5] = {-0.50000000000000000000000000000000000000, -0.32732683535398857189914622812342917778,
                              0.00000000000000000000000000000000000000, 0.32732683535398857189914622812342917778,
                              0.50000000000000000000000000000000000000};
const double h_gll5_wts[5] = {0.050000000000000000000000000000000000000, 0.27222222222222222222222222222222222222,
                              0.35555555555555555555555555555555555556, 0.27222222222222222222222222222222222222,
                              0.050000000000000000000000000000000000000};
const double h_gll9_pts[9] = {-0.50000000000000000000000000000000000000, -0.44987899770573007865617262220916897903,
                              -0.33859313975536887672294271354567122536, -0.18155873191308907935537603435432960651,
                              0.00000000000000000000000000000000000000, 0.18155873191308907935537603435432960651,
                              0.33859313975536887672294271354567122536, 0.44987899770573007865617262220916897903,
                              0.50000000000000000000000000000000000000};
const double h_gll9_wts[9] = {0.013888888888888888888888888888888888889, 0.082747680780402762523169860014604152919,
                              0.13726935625008086764035280928968636297, 0.17321425548652317255756576606985914397,
                              0.18575963718820861678004535147392290249, 0.17321425548652317255756576606985914397,
                              0.13726935625008086764035280928968636297, 0.082747680780402762523169860014604152919,
                              0.013888888888888888888888888888888888889};
const double h_gl3_pts[3] = {0.112701665379258311482073460022, 0.500000000000000000000000000000, 0.887298334620741688517926539980};
const double h_gl3_wts[3] = {0.277777777777777777777777777779, 0.444444444444444444444444444444, 0.277777777777777777777777777779};

} // namespace

extern "C" int mw_dycore_init(mw_dycore_t d, int init_data, double *rho_d, double *u, double *v, double *w, double *temp,
                              double *const *tracers) {
  if (!d) MW_FAIL("null handle");
  if (init_data < 0 || init_data > 3) MW_FAIL("ERROR: Invalid init_data");      // :1310
  CouplerPtrs c;
  if (make_coupler_ptrs(d, rho_d, u, v, w, temp, tracers, c)) return 1;
  mw_grid_t &g = d->g;
  g.latitude = 0;                                                                // :1249
  g.bc_x = MW_BC_PERIODIC; g.bc_y = MW_BC_PERIODIC; g.bc_z = MW_BC_WALL;         // :1332-1334, 1340-1342, 1423-1425, 1551-1553
  g.use_immersed = (init_data == MW_DATA_CITY || init_data == MW_DATA_BUILDING); // :1312, 1426, 1554
  d->etime = 0;                                                                  // :1317
  const int nz = g.nz, nens = g.nens, ord = d->ord;               // `ord` GLL points per cell (:1725-1727)
  const double dz = g.zlen / g.nz, dx = g.xlen / g.nx_glob;
  const double h_gll3_pts[3] = {-0.50000000000000000000000000000000000000, 0.00000000000000000000000000000000000000, 0.50000000000000000000000000000000000000};   // TransformMatrices.h:83-88
  const double h_gll3_wts[3] = {0.16666666666666666666666666666666666667, 0.66666666666666666666666666666666666667, 0.16666666666666666666666666666666666667};   // :90-95
  const double h_gll7_pts[7] = MW_GLL7_PTS, h_gll7_wts[7] = MW_GLL7_WTS;
  const double *h_gllN_pts = (ord == 3) ? h_gll3_pts : (ord == 7) ? h_gll7_pts : (ord == 9) ? h_gll9_pts : h_gll5_pts;
  const double *h_gllN_wts = (ord == 3) ? h_gll3_wts : (ord == 7) ? h_gll7_wts : (ord == 9) ? h_gll9_wts : h_gll5_wts;
  size_t nzc = (size_t)nz * nens, nze = (size_t)(nz + 1) * nens;
  double *hyc = d->hy_host.data(), *hytc = hyc + nzc, *hye = hyc + 2 * nzc, *hyte = hye + nze;
  std::vector<double> gllcols;     // supercell: hyDensGLL | hyDensThetaGLL | hyDensVapGLL, each (nz,5)
  InitP q;  memset(&q, 0, sizeof(q));
  q.init_data = init_data; q.i_beg = g.i_beg; q.j_beg = g.j_beg; q.xlen = g.xlen; q.ylen = g.ylen; q.cp_d = g.cp_d; q.p0 = g.p0;
  q.nx_glob = g.nx_glob; q.ny_glob = g.ny_glob; q.ord = ord;
  std::vector<double> bheights;
  if (init_data == MW_DATA_SUPERCELL) {                                          // init_supercell, :1687-1840
    const double z_0 = 0, z_trop = 12000, T_0 = 300, T_trop = 213, T_top = 213, p_0 = 100000;
    const double R_d = g.R_d, R_v = g.R_v, grav = g.grav, gamma = g.gamma_d, C0 = g.C0, ztop = g.zlen;
    std::vector<double> quad_temp((size_t)nz * (ord - 1) * ord), hyP((size_t)nz * ord);
    gllcols.assign((size_t)3 * nz * ord, 0.0);
    double *hyDensGLL = gllcols.data(), *hyDensThetaGLL = hyDensGLL + (size_t)nz * ord, *hyDensVapGLL = hyDensThetaGLL + (size_t)nz * ord;
    for (int k = 0; k < nz; k++) for (int kk = 0; kk < ord - 1; kk++) for (int kkk = 0; kkk < ord; kkk++) {       // :1736-1756
      double cellmid = (k + 0.5) * dz;
      double ord_b = cellmid + h_gllN_pts[kk] * dz, ord_t = cellmid + h_gllN_pts[kk + 1] * dz;
      double ord_m = 0.5 * (ord_b + ord_t);
      double ord_dz = dz * (h_gllN_pts[kk + 1] - h_gllN_pts[kk]);
      double zloc = ord_m + ord_dz * h_gllN_pts[kkk];
      double T = h_supercell_temperature(zloc, z_0, z_trop, ztop, T_0, T_trop, T_top);
      double press_dry = h_supercell_pressure_dry(zloc, z_0, z_trop, ztop, T_0, T_trop, T_top, p_0, R_d, grav);
      double qvs = h_supercell_sat_mix_dry(press_dry, T);
      double relhum = h_supercell_relhum(zloc, z_0, z_trop);
      if (relhum * qvs > 0.014) relhum = 0.014 / qvs;
      double qv = std::min(0.014, qvs * relhum);
      quad_temp[((size_t)k * (ord - 1) + kk) * ord + kkk] = -(1 + qv) * grav / (R_d + qv * R_v) / T;
    }
    hyP[0] = p_0;                                                                                                   // :1759-1774
    for (int k = 0; k < nz; k++) for (int kk = 0; kk < ord - 1; kk++) {
      double tot = 0;
      for (int kkk = 0; kkk < ord; kkk++) tot += quad_temp[((size_t)k * (ord - 1) + kk) * ord + kkk] * h_gllN_wts[kkk];
      tot *= dz * (h_gllN_pts[kk + 1] - h_gllN_pts[kk]);
      hyP[(size_t)k * ord + kk + 1] = hyP[(size_t)k * ord + kk] * exp(tot);
      if (kk == ord - 2 && k < nz - 1) hyP[(size_t)(k + 1) * ord] = hyP[(size_t)k * ord + ord - 1];
    }
    for (int k = 0; k < nz; k++) for (int kk = 0; kk < ord; kk++) {                                               // :1777-1805
      double zloc = (k + 0.5) * dz + h_gllN_pts[kk] * dz;
      double T = h_supercell_temperature(zloc, z_0, z_trop, ztop, T_0, T_trop, T_top);
      double press_tmp = h_supercell_pressure_dry(zloc, z_0, z_trop, ztop, T_0, T_trop, T_top, p_0, R_d, grav);
      double qvs = h_supercell_sat_mix_dry(press_tmp, T);
      double relhum = h_supercell_relhum(zloc, z_0, z_trop);
      if (relhum * qvs > 0.014) relhum = 0.014 / qvs;
      double qv = std::min(0.014, qvs * relhum);
      double press = hyP[(size_t)k * ord + kk];
      double dens_dry = press / (R_d + qv * R_v) / T;
      double dens_vap = qv * dens_dry;
      double dens = dens_dry + dens_vap;
      double dens_theta = pow(press / C0, 1.0 / gamma);
      hyDensGLL[(size_t)k * ord + kk] = dens; hyDensThetaGLL[(size_t)k * ord + kk] = dens_theta; hyDensVapGLL[(size_t)k * ord + kk] = dens_vap;
      if (kk == 0) for (int e = 0; e < nens; e++) { hye[(size_t)k * nens + e] = dens; hyte[(size_t)k * nens + e] = dens_theta; }
      if (k == nz - 1 && kk == ord - 1) for (int e = 0; e < nens; e++) { hye[(size_t)(k + 1) * nens + e] = dens; hyte[(size_t)(k + 1) * nens + e] = dens_theta; }
    }
    for (int k = 0; k < nz; k++) {                                                                                  // :1808-1840
      double dens_tot = 0, dens_theta_tot = 0;
      for (int kk = 0; kk < ord; kk++) { dens_tot += hyDensGLL[(size_t)k * ord + kk] * h_gllN_wts[kk];
                                         dens_theta_tot += hyDensThetaGLL[(size_t)k * ord + kk] * h_gllN_wts[kk]; }
      for (int e = 0; e < nens; e++) { hyc[(size_t)k * nens + e] = dens_tot; hytc[(size_t)k * nens + e] = dens_theta_tot; }
    }
  } else {
    bool use_hydro = (init_data == MW_DATA_THERMAL) || g.enable_gravity;
    if (use_hydro) {                                                             // :1396-1419, 1516-1541, 1620-1645
      const int nq = (init_data == MW_DATA_THERMAL) ? 3 : 9;
      const double *qp = (init_data == MW_DATA_THERMAL) ? h_gl3_pts : h_gll9_pts;
      const double *qw = (init_data == MW_DATA_THERMAL) ? h_gl3_wts : h_gll9_wts;
      for (int k = 0; k < nz; k++) for (int e = 0; e < nens; e++) {
        hyc[(size_t)k * nens + e] = 0.; hytc[(size_t)k * nens + e] = 0.;
        for (int kk = 0; kk < nq; kk++) {
          double z = (k + 0.5) * dz + (qp[kk] - 0.5) * dz;
          double hr, ht;
          h_hydro_const_theta(z, g.grav, g.C0, g.cp_d, g.p0, g.gamma_d, g.R_d, hr, ht);
          hyc[(size_t)k * nens + e] += hr * qw[kk];
          hytc[(size_t)k * nens + e] += hr * ht * qw[kk];
        }
      }
      for (int k = 0; k < nz + 1; k++) for (int e = 0; e < nens; e++) {
        double z = k * dz, hr, ht;
        h_hydro_const_theta(z, g.grav, g.C0, g.cp_d, g.p0, g.gamma_d, g.R_d, hr, ht);
        hye[(size_t)k * nens + e] = hr; hyte[(size_t)k * nens + e] = hr * ht;
      }
    } else {                                                                     // :1542-1547, 1646-1651
      for (size_t n = 0; n < nzc; n++) { hyc[n] = 1.15; hytc[n] = 1.15 * 300; }
      for (size_t n = 0; n < nze; n++) { hye[n] = 1.15; hyte[n] = 1.15 * 300; }
    }
    if (init_data == MW_DATA_CITY) {                                             // :1429-1452
      int building_length = 30;
      q.cells_per_building = (int)std::round(building_length / dx);
      q.buildings_pad = 20;
      q.nblocks_x = (static_cast<int>(g.xlen) / building_length - 2 * q.buildings_pad) / 3;
      q.nblocks_y = (static_cast<int>(g.ylen) / building_length - 2 * q.buildings_pad) / 9;
      q.nbx = q.nblocks_x * 3; q.nby = q.nblocks_y * 9;
      if (q.cells_per_building < 1) MW_FAIL("city init: dx too coarse for 30 m buildings");
      bheights.assign((size_t)std::max(1, q.nbx * q.nby), 0.0);
      std::mt19937 gen{17};
      std::normal_distribution<> dist{60, 10};
      for (int j = 0; j < q.nby; j++) for (int i = 0; i < q.nbx; i++) bheights[(size_t)j * q.nbx + i] = dist(gen);
    }
  }
  if (upload_background(d)) return 1;
  fill_params(d);
  double *dev_cols = nullptr, *dev_bh = nullptr;
  if (!gllcols.empty()) {
    MW_HIP(hipMalloc(&dev_cols, gllcols.size() * 8));
    MW_HIP(hipMemcpy(dev_cols, gllcols.data(), gllcols.size() * 8, hipMemcpyHostToDevice));
    q.hyDensGLL = dev_cols; q.hyDensThetaGLL = dev_cols + (size_t)nz * ord; q.hyDensVapGLL = dev_cols + (size_t)2 * nz * ord;
  }
  if (!bheights.empty()) {
    MW_HIP(hipMalloc(&dev_bh, bheights.size() * 8));
    MW_HIP(hipMemcpy(dev_bh, bheights.data(), bheights.size() * 8, hipMemcpyHostToDevice));
    q.bheights = dev_bh;
  }
  MW_HIP(hipMemsetAsync(d->imm, 0, (size_t)d->p.nC * 8, d->stream));                    // :1315
  const DyP &p = d->p;
  MW_KLAUNCH(k_init_cells, plane_grid((long long)p.ny * p.nx * p.nens, p.nz), dim3(256), 0, d->stream, p, q, c, d->imm);
  MW_LAUNCH_CHECK();
  MW_HIP(hipStreamSynchronize(d->stream));
  if (dev_cols) (void)hipFree(dev_cols);
  if (dev_bh) (void)hipFree(dev_bh);
  // the six flux arrays start at zero (:1677-1682)
  MW_HIP(hipMemsetAsync(d->FX, 0, (size_t)p.V * p.fxV * 8, d->stream));
  MW_HIP(hipMemsetAsync(d->FY, 0, (size_t)p.V * p.fyV * 8, d->stream));
  MW_HIP(hipMemsetAsync(d->FZ, 0, (size_t)p.V * p.fzV * 8, d->stream));
  return 0;
}

extern "C" {

int mw_perturb_temperature(const mw_grid_t *g, double *temp, void *stream) {
  if (!g || !temp) MW_FAIL("null argument");
  long long n = (long long)g->nz * g->ny * g->nx * g->nens;
  MW_KLAUNCH(k_perturb_temperature, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g->nz, g->ny, g->nx,
                     g->nens, g->i_beg, g->j_beg, g->xlen / g->nx_glob, g->ylen / g->ny_glob, g->zlen / g->nz, g->xlen, g->ylen, temp);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_perturb_temperature_random(const mw_grid_t *g, double *temp, void *stream) {
  if (!g || !temp) MW_FAIL("null argument");
  const int num_levels = g->nz / 4;
  const long long ncol = (long long)g->ny * g->nx * g->nens;
  if (num_levels < 1) return 0;
  const unsigned long long myrank = (unsigned long long)g->py * g->nproc_x + g->px;
  const unsigned long long seed = myrank * (unsigned long long)g->nz * g->nx * g->ny * g->nens;
  const long long n = (long long)num_levels * ncol;
  MW_KLAUNCH(k_perturb_temperature_random, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, num_levels, ncol, seed, temp);
  MW_LAUNCH_CHECK();
  return 0;
}

} // extern "C"
