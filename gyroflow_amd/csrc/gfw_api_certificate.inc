// gfw_api_certificate.inc — the first pass's certificate on the host: the s(rho) table, the derived bounds on s and its derivatives, the coefficients of E
// (included by gfw_api.hip: one translation unit.  DESIGN.md section 2c)
// s(rho) = theta_d(atan(r)) / r with r = sqrt(rho) (opencv_fisheye.rs:72-95), tabulated for the certified first pass.
static double p1_s_of_rho(double rho, const float *k) {
    // all four k zero: the reference skips the atan scaling altogether and returns (x/z, y/z) (opencv_fisheye.rs:75),
    // which the exact path honours through k_all_zero — the table must describe the same map, s == 1
    if (k[0] == 0.0f && k[1] == 0.0f && k[2] == 0.0f && k[3] == 0.0f) return 1.0;
    const double r = sqrt(rho);
    if (r == 0.0) return 1.0;
    const double t = atan(r), t2 = t * t;
    return t * (1.0 + t2 * ((double)k[0] + t2 * ((double)k[1] + t2 * ((double)k[2] + t2 * (double)k[3])))) / r;
}
// ---- derivative bounds of s(rho), derived (round 5; DESIGN.md section 2c) -------------------------------------------------------------------------
// s = A(rho) P(w):  A(rho) = atan(sqrt rho) / sqrt rho = int_0^1 dt / (1 + rho t^2),  w(rho) = atan^2(sqrt rho) = rho A^2 (= theta^2),
// P(w) = 1 + k0 w + k1 w^2 + k2 w^3 + k3 w^4.  From the integral: |d^n A / d rho^n| <= n! / (2n + 1) for every rho >= 0 (A, -A', A'', ... are positive and
// decreasing);  w' = A / (1 + rho) in (0, 1],  w'' = A' / (1 + rho) - A / (1 + rho)^2,  w(3) = A'' / (1 + rho) - 2 A' / (1 + rho)^2 + 2 A / (1 + rho)^3:
// |w''| <= 4/3, |w(3)| <= 46/15.  The values of s', s'' at a point come from the closed forms below (a series under rho = 1/64, where the closed forms
// cancel); between two points of a grid of spacing g the next derivative's GLOBAL bound (products of the bounds above) carries the value:
// |s''(rho)| <= |s''(rho_i)| + g L3 on [rho_i, rho_i + g].  Nothing here is sampled-and-doubled: every number the certificate uses is a bound.
static void p1_A_derivs(double rho, double &A, double &A1, double &A2) {
    if (rho < 1.0 / 64.0) {                     // alternating series, terms falling by >= 64 each: 14 terms leave < 2^-84
        A = A1 = A2 = 0.0;
        double pw = 1.0;                         // (-rho)^n
        for (int n = 0; n < 14; ++n) { A += pw / (2 * n + 1); pw *= -rho; }
        double p1 = 1.0;                         // (-rho)^(n-1)
        for (int n = 1; n < 14; ++n) { A1 += -(double)n / (2 * n + 1) * p1; p1 *= -rho; }
        double p2 = 1.0;                         // (-rho)^(n-2)
        for (int n = 2; n < 14; ++n) { A2 += (double)n * (n - 1) / (2 * n + 1) * p2; p2 *= -rho; }
        return;
    }
    const double r = sqrt(rho);
    A = atan(r) / r;
    A1 = (1.0 / (1.0 + rho) - A) / (2.0 * rho);                               // from (rho A^2)' = A / (1 + rho)
    A2 = (-1.0 / ((1.0 + rho) * (1.0 + rho)) - 3.0 * A1) / (2.0 * rho);       // the same identity differentiated once more
}
struct P1Derivs { double s, s1, s2; };
static P1Derivs p1_s_derivs(double rho, const float *k) {
    double A, A1, A2;
    p1_A_derivs(rho, A, A1, A2);
    const double w = rho * A * A, w1 = A / (1.0 + rho), w2 = A1 / (1.0 + rho) - A / ((1.0 + rho) * (1.0 + rho));
    const double k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3];
    const double P = 1.0 + w * (k0 + w * (k1 + w * (k2 + w * k3)));
    const double P1 = k0 + w * (2.0 * k1 + w * (3.0 * k2 + w * 4.0 * k3));
    const double P2 = 2.0 * k1 + w * (6.0 * k2 + w * 12.0 * k3);
    P1Derivs d;
    d.s = A * P;
    d.s1 = A1 * P + A * P1 * w1;
    d.s2 = A2 * P + 2.0 * A1 * P1 * w1 + A * (P2 * w1 * w1 + P1 * w2);
    return d;
}
// The table lives in one buffer per context, d_p1_table.  Frames held for a clip launch (a ClipBatch: gfw_api_clip.inc) read it when that launch goes out, with the
// range constants of the table they were set up against: a rebuild sends them on their way first (as ck_table does), and stream order puts the copy behind them.
// The functions below return that launch's error — the frame's — or GFW_OK; whether there is a table, and a certified pass, they answer beside it.
struct ClipBatch;
static void clip_envelope(const ClipBatch *b, double &hx, double &hy);      // (gfw_api_clip.inc)
static int clip_flush(gfw_ctx *c, ClipBatch *b);
// A new table takes the buffer's place.  `moved`: it is there (always on a dry context, where there is no buffer); else the frame takes the exact first pass.
static int p1_table_upload(gfw_ctx *c, const std::vector<float2> &tab, ClipBatch *pending, bool &moved) {
    moved = c->dry;
    if (c->dry) return GFW_OK;
    { const int frc = clip_flush(c, pending); if (frc != GFW_OK) return frc; }      // (a pending launch names the table that is about to move)
    const size_t bytes = (GFW_P1_TABLE_N + 1) * sizeof(float2);
    moved = c->d_p1_table.ensure(bytes) == hipSuccess && hipMemcpyAsync(c->d_p1_table.ptr, tab.data(), bytes, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
            hipStreamSynchronize(c->stream) == hipSuccess;                         // (`tab` is a stack-lifetime source)
    return GFW_OK;
}
static int p1_prepare_table(gfw_ctx *c, const gfw_kernel_params &p, float rho_max, ClipBatch *pending, bool &ready) {      // ready: the context's table serves these coefficients and this range
    ready = c->p1_valid && memcmp(c->p1_k, p.k, sizeof(c->p1_k)) == 0 && rho_max <= c->p1_rho_max && rho_max >= 0.5f * c->p1_rho_max;
    if (ready) return GFW_OK;
    const int N = GFW_P1_TABLE_N;
    std::vector<float2> tab(N + 1);
    const double h = (double)rho_max / N;
    double s_prev = p1_s_of_rho(0.0, p.k);
    for (int i = 0; i < N; ++i) {
        const double s_next = p1_s_of_rho((i + 1) * h, p.k);
        tab[i] = float2{(float)s_prev, (float)(s_next - s_prev)};
        s_prev = s_next;
    }
    tab[N] = float2{(float)s_prev, 0.0f};
    const bool k_zero = p.k[0] == 0.0f && p.k[1] == 0.0f && p.k[2] == 0.0f && p.k[3] == 0.0f;
    // global bounds over [0, rho_max]: P and its derivatives over w in [0, w_max] by the triangle inequality, then the products (header comment)
    double smax = 1.0, slope = 0.0, s2max = 0.0, u1 = 0.0, u2 = 0.0, t32 = 0.0;
    double kappa = 3.0;                                             // all four k zero: the exact path is (X/W) * f + c, s == 1, every derivative 0
    if (!k_zero) {
        const double tmax = atan(sqrt((double)rho_max)), wm = tmax * tmax;
        const double a0 = fabs((double)p.k[0]), a1 = fabs((double)p.k[1]), a2 = fabs((double)p.k[2]), a3 = fabs((double)p.k[3]);
        const double P0 = 1.0 + wm * (a0 + wm * (a1 + wm * (a2 + wm * a3)));
        const double Pd1 = a0 + wm * (2.0 * a1 + wm * (3.0 * a2 + wm * 4.0 * a3));
        const double Pd2 = 2.0 * a1 + wm * (6.0 * a2 + wm * 12.0 * a3);
        const double Pd3 = 6.0 * a2 + wm * 24.0 * a3;
        const double L1 = P0 / 3.0 + Pd1;                                                   // |s'|   <= |A'| P + A |P'| w'
        const double L2 = 0.4 * P0 + 2.0 * Pd1 + Pd2;                                       // |s''|  <= |A''| P + 2 |A'| |P'| w' + A (|P''| w'^2 + |P'| |w''|)
        const double L3 = (6.0 / 7.0) * P0 + 1.2 * Pd1 + (Pd2 + Pd1 * 4.0 / 3.0)            // |s(3)| <= |A(3)| P + 3 |A''| |(P)'| + 3 |A'| |(P)''| + A |(P)(3)|
                        + (Pd3 + 4.0 * Pd2 + Pd1 * 46.0 / 15.0);
        const int NG = 4096;
        const double g = (double)rho_max / NG;
        smax = 0.0;
        for (int i = 0; i < NG; ++i) {
            const P1Derivs d = p1_s_derivs(i * g, p.k);
            const double hi = (i + 1) * g;
            const double b0 = fabs(d.s) + g * L1, b1 = fabs(d.s1) + g * L2, b2 = fabs(d.s2) + g * L3;     // bounds over [i g, (i + 1) g]
            smax = fmax(smax, b0); slope = fmax(slope, b1); s2max = fmax(s2max, b2);
            u1 = fmax(u1, sqrt(hi) * b1); u2 = fmax(u2, hi * b1); t32 = fmax(t32, hi * sqrt(hi) * b2);
        }
        const double slack = 1.0 + 1e-9;                            // the f64 evaluation itself
        smax *= slack; slope *= slack; s2max *= slack; u1 *= slack; u2 *= slack; t32 *= slack;
        // the exact path's theta_d / r as a function of its (already rounded) rho: sqrt (1 rounding), glibc atanf (< 1 ulp = 2 roundings), the polynomial
        // 1 + k0 t^2 + k1 t^4 + k2 t^6 + k3 t^8 (powers by repeated products: 2, 4, 6, 8 roundings on the terms, 4 on the partial sums), t * poly, / r:
        // relative error <= u * kappa, kappa = 3.5 (1 + R) + (R + 4 K) + 3 with R = max sum (2i |k_i| t^2i) / |P| (both t P'/P's bound and the terms' own
        // roundings) and K = max sum |terms| / |P| (the partial sums)  (DESIGN.md section 2c).  |P| from below: its value on a grid of w = t^2 less the
        // grid step times the bound on |dP/dw|; the sums of absolute terms at the interval's upper end.
        double rp = 0.0, kp = 1.0;
        const double gw = wm / 4096.0;
        for (int i = 0; i <= 4096; ++i) {
            const double t2 = gw * i, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double P = fabs(1.0 + p.k[0] * t2 + p.k[1] * t4 + p.k[2] * t6 + p.k[3] * t8) - gw * Pd1;
            const double t2h = t2 + gw, t4h = t2h * t2h, t6h = t4h * t2h, t8h = t4h * t4h;
            const double Pabs = 1.0 + a0 * t2h + a1 * t4h + a2 * t6h + a3 * t8h;
            const double dPabs = 2.0 * a0 * t2h + 4.0 * a1 * t4h + 6.0 * a2 * t6h + 8.0 * a3 * t8h;
            if (!(P > 1e-3)) { rp = kp = 1e30; break; }           // theta_d's polynomial (nearly) vanishes inside the range: no certificate
            rp = fmax(rp, dPabs / P); kp = fmax(kp, Pabs / P);
        }
        kappa = 4.5 * rp + 4.0 * kp + 6.5;
    }
    // the table's own error against s: the chord of a function with |s''| <= s2max over an interval h, the float rounding of the entry s_i (u |s|) and of
    // the entry s_{i+1} - s_i (u h |s'|, times a fraction <= 1); the fma that combines them is counted with the first pass's roundings (section 2c, item 4)
    const double etab = h * h / 8.0 * s2max + (smax + h * slope) / 16777216.0;
    if (!(etab == etab) || !(smax == smax) || !(slope == slope) || !(kappa == kappa) || !(t32 == t32)) { c->p1_valid = false; return GFW_OK; }
    { bool moved; const int rc = p1_table_upload(c, tab, pending, moved); if (rc != GFW_OK || !moved) return rc; }
    memcpy(c->p1_k, p.k, sizeof(c->p1_k));
    c->p1_rho_max = rho_max; c->p1_etab = etab; c->p1_smax = smax; c->p1_slope = slope; c->p1_kappa = kappa; c->p1_valid = true;
    c->p1_u1 = u1; c->p1_u2 = u2; c->p1_t32 = t32;
    ready = true;
    return GFW_OK;
}
// ---- radial models other than the fisheye (round 6): GoPro's inverted polynomial --------------------------------------------------------------------------------
// gopro.rs:25-72: distort_point scales (x/z, y/z) by T(r) = k1 q(theta) / r with theta = atan r (r below tan 89 degrees) and q = POLY^-1, POLY(p) = sum k_i p^i,
// found by ten Newton steps from the paraxial guess (theta - k0) / k1 that stop once a step is below 1e-7.  The first pass evaluates that for EVERY pixel only to
// round it to a matrix row; the certified pass replaces it by a table of T over r (POLY has even powers: T is smooth in r, not in rho = r^2 — gfw_frame.hip p1_key)
// and hands the pixels within E of a half-integer to the exact code, like the fisheye's.  What the certificate needs, all of it bounds:
//   * the iterates' interval I = [-e0, p_hi + e0], p_hi = q(theta_max) (+ 2 %), e0 >= |paraxial guess - root| (a grid over theta + its Lipschitz slack);
//     on I: d_min <= POLY' and |POLY''| <= M2 from grid values and the next derivative's bound, POLY' <= d_max and |POLY'''| <= M3 by the triangle inequality;
//   * Newton: an error e becomes at most c e^2, c = M2 / (2 d_min); c e0 <= 1/2 keeps every iterate within e0 of the root (inside I) and halves the error at least
//     every step.  In float every step adds noise of at most nu = (12.1 u A + u |p|) / d_min + 1.01 u |p| (Horner of seven terms: gamma_12 A, A = sum |k_i| |p|^i;
//     the quotient and the subtraction), so the next error is at most e / 2 + nu.  Whether the loop leaves on a small step (|fix| < 1e-7: the error before the step
//     was <= 2 (1e-7 + nu), after it <= 4 c (1e-7 + nu)^2 + nu) or after ten steps (<= e0 / 2^10 squared away + 2 nu), the p it returns is within 2.01 nu + 1e-13 of
//     the root of POLY(p) = theta~ for the theta~ it was given; theta~ itself (sqrt 2u on r, glibc atanf < 1 ulp) is within 4 u theta of atan r: 4 u theta / d_min more.
//   * T(r) = G(w(r)) A(r), w = atan r, A = w / r, G(w) = Q(w) / w = int_0^1 Q'(t w) dt with Q = k1 q: |Q'| <= k1 / d_min = Q1, |Q''| <= k1 M2 / d_min^3 = Q2,
//     |Q'''| <= k1 (3 M2^2 + d_max M3) / d_min^5 = Q3, so |G| <= Q1, |G'| <= Q2 / 2, |G''| <= Q3 / 3; |A| <= 1, |A'| <= 0.325, |A''| <= 2/3, w' <= 1, |w''| <= 0.65:
//     |T''| <= Q3 / 3 + 0.325 Q2 + 0.65 Q2 / 2 + 2 Q1 / 3 = T2 (global, loose: it only prices the chord of a table interval and the slack below);
//     |T'| <= max_i |T(r_i+1) - T(r_i)| / g + g T2 / 2 over a grid of NG intervals (mean value theorem + the Lipschitz bound on T'), T from f64 Newton;
//     |T| <= max_i T(r_i) + g T1.
// The lattice form would need the curvature of T as tightly as the fisheye's; the per-pixel form (55 issue slots against the exact pass's Newton loop) does not,
// and is what these clips take (p1_lat[5] = 1).
struct P1Radial { bool ok = false; int model = 0; float k[12] = {}; double r_max = 0, Tmax = 1, T1 = 0, T2 = 0, etab = 0, nu2 = 0, dmin = 0; };
// What every radial model's certificate shares, given its scale T(r) as an f64 function, a global bound T2 >= |T''| on [0, r_max] (loose is fine) and nu2, the bound on
// the exact path's |r_norm~ - r T(r)| beyond its last roundings: max |T'| from differences of values on a grid plus half a step times T2 (mean value theorem + the
// Lipschitz bound on T'), max |T| likewise, the table (T_i, T_i+1 - T_i) over N intervals and its chord error — sampled at the seven inner eighths of every interval,
// where the difference to the chord is taken directly; between two such points it strays from its own chord by at most (h / 8)^2 / 8 T2: the loose T2 prices a 64th
// of what it would over the whole interval.
template <typename F>
static bool p1_radial_finish(const gfw_kernel_params &p, double r_max, F T, double T2, double nu2, P1Radial &R, std::vector<float2> *tab_out) {
    const int N = GFW_P1_TABLE_N, NG = 16384;
    const double u = 1.0 / 16777216.0, g = r_max / NG, h = r_max / N;
    if (!(T2 == T2) || !(nu2 == nu2) || !(T2 < 1e12)) return false;
    double T1 = 0.0, Tmax = 0.0, prev = T(0.0);
    for (int i = 1; i <= NG; ++i) {
        const double t = T(g * i);
        if (!(t == t) || !(fabs(t) < 1e6)) return false;
        T1 = fmax(T1, fabs(t - prev) / g); Tmax = fmax(Tmax, fmax(fabs(t), fabs(prev))); prev = t;
    }
    T1 = T1 * (1.0 + 1e-9) + 0.5 * g * T2 + 1e-9 / g;                                       // (+ the f64 evaluation of two neighbouring values)
    Tmax = Tmax * (1.0 + 1e-9) + g * T1;
    std::vector<double> node(N + 1);
    for (int i = 0; i <= N; ++i) node[i] = T(h * i);
    double chord = 0.0;
    for (int i = 0; i < N; ++i)
        for (int j = 1; j < 8; ++j) chord = fmax(chord, fabs(T(h * i + h * j / 8.0) - (node[i] + (node[i + 1] - node[i]) * j / 8.0)));
    memcpy(R.k, p.k, sizeof(R.k)); R.r_max = r_max; R.Tmax = Tmax; R.T1 = T1; R.T2 = T2; R.nu2 = nu2;
    R.etab = chord * (1.0 + 1e-9) + 1e-12 + (h / 8.0) * (h / 8.0) / 8.0 * T2 + u * (2.0 * Tmax + h * T1);
    if (tab_out) {
        tab_out->resize(N + 1);
        for (int i = 0; i < N; ++i) (*tab_out)[i] = float2{(float)node[i], (float)(node[i + 1] - node[i])};
        (*tab_out)[N] = float2{(float)node[N], 0.0f};
    }
    R.ok = true;
    return true;
}
static double p1_gopro_q(double theta, const double *k) {             // the root of POLY(p) = theta in f64 (Newton to the last bit)
    double p = theta / k[1];
    for (int it = 0; it < 60; ++it) {
        double e = 0, d = 0;
        for (int i = 6; i >= 0; --i) { d = d * p + e; e = e * p + k[i]; }
        const double fix = (e - theta) / d;
        p -= fix;
        if (fabs(fix) < 1e-16 * fmax(1.0, fabs(p))) break;
    }
    return p;
}
static bool p1_prepare_radial_gopro(const gfw_kernel_params &p, double r_max, P1Radial &R, std::vector<float2> *tab_out) {
    R.ok = false;
    double k[7]; for (int i = 0; i < 7; ++i) k[i] = (double)p.k[i];
    if (k[0] != 0.0 || !(k[1] > 1e-3) || !(r_max > 0.0) || r_max > 8.0) return false;          // (k0 != 0: r_norm does not vanish at the centre, T has a pole there)
    const double theta_max = atan(r_max);
    double p_hi = p1_gopro_q(theta_max, k);
    if (!(p_hi > 0.0) || !(p_hi < 16.0)) return false;
    { double chk = 0; for (int i = 6; i >= 0; --i) chk = chk * p_hi + k[i]; if (!(fabs(chk - theta_max) < 1e-9)) return false; }      // the f64 solve itself converged
    const double p_root_max = p_hi;
    p_hi = p_hi * 1.02 + 1e-3;
    // e0 >= |paraxial guess - root| over the range: a grid of theta; between grid points the difference moves by at most (1 / k1 + 1 / d) per unit of theta, d >= 0.05
    // being required of POLY' below (checked on the interval this e0 defines: a failure there voids the certificate, never loosens it)
    double e0 = 0.0;
    { const int NE = 2048; const double gt = theta_max / NE;
      for (int i = 0; i <= NE; ++i) { const double th = gt * i; e0 = fmax(e0, fabs(th / k[1] - p1_gopro_q(th, k))); }
      e0 += 0.5 * gt * (1.0 / k[1] + 1.0 / 0.05); }
    const double lo = -e0 - 1e-3, hi = fmax(p_hi, theta_max / k[1]) + e0 + 1e-3, P = fmax(fabs(lo), fabs(hi));
    (void)p_root_max;
    double M3 = 0, dmax = 0, Amax = 0;
    { double pw1 = 1, pw2 = 1, pwA = 1;               // P^(i-3), P^(i-1), P^i
      for (int i = 0; i < 7; ++i) { Amax += fabs(k[i]) * pwA; pwA *= P; }
      for (int i = 1; i < 7; ++i) { dmax += i * fabs(k[i]) * pw2; pw2 *= P; }
      for (int i = 3; i < 7; ++i) { M3 += (double)i * (i - 1) * (i - 2) * fabs(k[i]) * pw1; pw1 *= P; } }
    // POLY' from below and |POLY''| from above over the iterates' interval: values on a grid, and between two grid points the next derivative's bound carries them
    // (the triangle inequality alone overstates |POLY''| of a typical lens sixfold — its terms alternate in sign — and with it the Newton constant)
    const int ND = 8192;
    const double gd = (hi - lo) / ND;
    double dmin = 1e300, M2 = 0.0;
    for (int i = 0; i <= ND; ++i) {
        const double x = lo + gd * i;
        double d = 0, d2 = 0;
        for (int j = 6; j >= 1; --j) d = d * x + j * k[j];
        for (int j = 6; j >= 2; --j) d2 = d2 * x + (double)j * (j - 1) * k[j];
        dmin = fmin(dmin, d); M2 = fmax(M2, fabs(d2));
    }
    M2 += 0.5 * gd * M3;
    dmin -= 0.5 * gd * M2;
    if (!(dmin > 0.05)) return false;                                                       // POLY (nearly) folds inside the range: no certificate
    const double cN = M2 / (2.0 * dmin);
    if (!(cN * e0 <= 0.5)) return false;                                                    // the Newton iteration is not provably contracting from the paraxial guess
    const double u = 1.0 / 16777216.0;
    const double nu = (12.1 * u * Amax + u * P) / dmin + 1.01 * u * P;
    const double Q1 = k[1] / dmin, Q2 = k[1] * M2 / (dmin * dmin * dmin), Q3 = k[1] * (3.0 * M2 * M2 + dmax * M3) / pow(dmin, 5.0);
    const double T2 = Q3 / 3.0 + 0.325 * Q2 + 0.65 * Q2 / 2.0 + 2.0 * Q1 / 3.0;
    const double nu2 = k[1] * (2.01 * nu + 1e-13 + 4.0 * u * theta_max / dmin);                    // |r_norm - k1 q(atan r)| of the exact path, beyond its last roundings
    R.dmin = dmin;
    return p1_radial_finish(p, r_max, [&](double r) { return r == 0.0 ? 1.0 : k[1] * p1_gopro_q(atan(r), k) / r; }, T2, nu2, R, tab_out);      // (T(0) = k1 / POLY'(0) = 1)
}
// ---- closed-form radial models (round 6): no iteration in the exact path, so the certificate is the table's (p1_radial_finish) plus the roundings of the formula ----
// sony.rs:69-88 and generic_polynomial.rs (the same with twelve coefficients): theta = atan r, theta_d = sum_i k_i theta^(i+1), scale = theta_d / r.
//   T(r) = Phi(theta) A(r), Phi = sum k_i theta^i, A = theta / r: |T''| <= F2 + 1.3 F1 + 2/3 F0 with F0, F1, F2 the triangle-inequality bounds of Phi, Phi', Phi'' on
//   [0, theta_max] (w' <= 1, |w''| <= 0.65, |A'| <= 0.325, |A''| <= 2/3 as for GoPro).  The float path forms the powers by products (t2 = t t, t3 = t2 t, t4 = t2 t2,
//   t5 = t2 t3, t6 = t3 t3, ...: theta^m carries (m - 1) roundings), multiplies by k (one more), adds left to right (n - 1 roundings on partial sums <= sum |terms|), from
//   a theta~ within 4 u theta of atan r (sqrt 2u, glibc atanf < 1 ulp): |theta_d~ - theta_d| <= 1.01 u (5 B + (n - 1) S), B = sum m |k_(m-1)| theta^m, S = sum |k_(m-1)| theta^m.
static bool p1_prepare_radial_thetapoly(const gfw_kernel_params &p, int n, double r_max, P1Radial &R, std::vector<float2> *tab_out) {
    R.ok = false;
    double k[12]; for (int i = 0; i < 12; ++i) k[i] = i < n ? (double)p.k[i] : 0.0;
    bool zero = true; for (int i = 0; i < (n == 6 ? 4 : 12); ++i) zero = zero && k[i] == 0.0;        // (the reference returns (x/z, y/z) untouched: sony.rs:71, generic_polynomial.rs)
    if (zero || !(r_max > 0.0) || r_max > 8.0) return false;
    const double tm = atan(r_max), u = 1.0 / 16777216.0;
    double F0 = 0, F1 = 0, F2 = 0, B = 0, S = 0, pw = 1.0;          // pw = tm^i
    for (int i = 0; i < n; ++i) {
        F0 += fabs(k[i]) * pw; if (i >= 1) F1 += i * fabs(k[i]) * pw / tm; if (i >= 2) F2 += (double)i * (i - 1) * fabs(k[i]) * pw / (tm * tm);
        B += (i + 1) * fabs(k[i]) * pw * tm; S += fabs(k[i]) * pw * tm; pw *= tm;
    }
    const double T2 = F2 + 1.3 * F1 + 2.0 / 3.0 * F0;
    const double nu2 = 1.01 * u * (5.0 * B + (n - 1) * S);
    return p1_radial_finish(p, r_max, [&](double r) {
        if (r == 0.0) return k[0];
        const double t = atan(r); double acc = 0.0; for (int i = n - 1; i >= 0; --i) acc = acc * t + k[i];
        return acc * t / r; }, T2, nu2, R, tab_out);
}
// poly3.rs / poly5.rs / ptlens.rs (lensfun's models): the scale is a polynomial in r itself — poly3 1 + k0 r^2, poly5 1 + k0 r^2 + k1 r^4, ptlens 1 + k2 r + k1 r^2 + k0 r^3
// — evaluated from rho~ = x x + y y (2u) and, for ptlens, r~ = sqrt(rho~) (2u): term roundings 3u (k rho, k r), 6u ((k rho) rho, (k rho) r), the additions 1u each on
// partial sums <= sum |terms|; r_norm = r scale, so nu2 = r_max times the scale's error.
static bool p1_prepare_radial_rpoly(const gfw_kernel_params &p, int model, double r_max, P1Radial &R, std::vector<float2> *tab_out) {
    R.ok = false;
    if (!(r_max > 0.0) || r_max > 8.0) return false;
    double c[5] = {1.0, 0, 0, 0, 0}, e[5] = {0, 0, 0, 0, 0}; int adds = 1;      // scale = sum c_j r^j; e_j: roundings on term j
    if (model == GFW_MODEL_POLY3) { c[2] = p.k[0]; e[2] = 3; adds = 1; }
    else if (model == GFW_MODEL_POLY5) { c[2] = p.k[0]; c[4] = p.k[1]; e[2] = 3; e[4] = 6; adds = 2; }
    else { c[3] = p.k[0]; c[2] = p.k[1]; c[1] = p.k[2]; e[3] = 6; e[2] = 3; e[1] = 3; adds = 3; }
    const double u = 1.0 / 16777216.0;
    double sum_abs = 0, err = 0, T2 = 0, pw = 1.0;
    for (int j = 0; j < 5; ++j) { sum_abs += fabs(c[j]) * pw; err += e[j] * fabs(c[j]) * pw; if (j >= 2) T2 += (double)j * (j - 1) * fabs(c[j]) * pw / (r_max * r_max); pw *= r_max; }
    const double nu2 = 1.01 * u * r_max * (err + adds * sum_abs);
    return p1_radial_finish(p, r_max, [&](double r) { return c[0] + r * (c[1] + r * (c[2] + r * (c[3] + r * c[4]))); }, T2 + 1e-12, nu2, R, tab_out);
}
static bool p1_prepare_radial(int model, const gfw_kernel_params &p, double r_max, P1Radial &R, std::vector<float2> *tab_out) {
    switch (model) {
    case GFW_MODEL_GOPRO: return p1_prepare_radial_gopro(p, r_max, R, tab_out);
    case GFW_MODEL_SONY: return p1_prepare_radial_thetapoly(p, 6, r_max, R, tab_out);
    case GFW_MODEL_GENERIC_POLYNOMIAL: return p1_prepare_radial_thetapoly(p, 12, r_max, R, tab_out);
    case GFW_MODEL_POLY3: case GFW_MODEL_POLY5: case GFW_MODEL_PTLENS: return p1_prepare_radial_rpoly(p, model, r_max, R, tab_out);
    default: return false;
    }
}
// Models with a radial certificate (gfw_debug_p1_radial, the interpreter's audits) ...
static bool p1_model_radial(int model) {
    return model == GFW_MODEL_GOPRO || model == GFW_MODEL_SONY || model == GFW_MODEL_GENERIC_POLYNOMIAL || model == GFW_MODEL_POLY3 || model == GFW_MODEL_POLY5 || model == GFW_MODEL_PTLENS;
}
// ... and those whose clips TAKE the certified pass: where the exact mid-row projection costs more than a square root and a table fetch.  Measured on the MI355X, C2
// geometry, us per frame exact -> certified (profiles/r06_radial_closed_form.txt): gopro 91.5 -> 70.2, generic_polynomial 64.9 -> see there, sony 61.6 -> 56.8;
// poly3 46.8 -> 50.1, poly5 47.2 -> 50.2, ptlens 48.4 -> 50.1 — a polynomial in r is cheaper than its own table.  (GFW_P1_RADIAL=all in the environment: every
// certified model, for A/B runs.)
static bool p1_model_radial_served(int model) {
    static const bool all = [] { const char *e = getenv("GFW_P1_RADIAL"); return e && strcmp(e, "all") == 0; }();
    return model == GFW_MODEL_GOPRO || model == GFW_MODEL_SONY || model == GFW_MODEL_GENERIC_POLYNOMIAL || (all && p1_model_radial(model));
}
static void p1_radial_free(gfw_ctx *c) { delete c->p1_radial; c->p1_radial = nullptr; }
// Audit mode (GFW_OPT_KERNEL_VARIANT 3 / 4): the launch counts certificates and checks each one.  False: no counters, the frame takes the exact pass.
static bool p1_attach_audit(gfw_ctx *c, GfwYuvArgs &Y) {
    if (c->kernel_variant != 3 && c->kernel_variant != 4) return true;
    if (c->dry) { Y.audit = &c->dry_audit; return true; }            // (gfw_debug_jit_key_clip_params: the key of the audit build, no device)
    if (audit_counters(c) != hipSuccess) return false;
    Y.audit = (unsigned long long *)c->d_audit.ptr;
    return true;
}
// What p1_setup and p1_setup_radial end on, E = e[0] + e[1] omega + e[2] mu derived: the kernel evaluates omega, mu from the matrix it actually uses; the host's own
// view of them — from the mid-row matrix, if it has one — only decides whether the certified pass is worth launching (the answer) and is what gfw_get_audit reports
static bool p1_finish(gfw_ctx *c, const gfw_kernel_params &p0, const float *h_matrices, int matrix_count, double rmax, const double e[3], GfwYuvArgs &Y) {
    const bool hrs = (p0.flags & GFW_FLAG_HORIZONTAL_RS) != 0;
    double omega = 1.0, mu = 6.0 * (rmax + 1.0);
    if (h_matrices) {
        const float *m = h_matrices + (size_t)(matrix_count >> 1) * 14;
        const double x0 = p0.translation2d[0], x1 = x0 + p0.output_width, y0 = p0.translation2d[1], y1 = y0 + p0.output_height;
        const double ax = fmax(fabs(x0), fabs(x1)), ay = fmax(fabs(y0), fabs(y1));
        const double px = ax * fabs(m[0]) + ay * fabs(m[1]), py = ax * fabs(m[3]) + ay * fabs(m[4]), pw = ax * fabs(m[6]) + ay * fabs(m[7]);
        const double wden = fmax((double)m[8] - pw, fmax(1.0 / 1024.0, (pw + fabs(m[8])) / 8.0));
        omega = 3.0 * pw / wden; mu = 3.0 * fmax(px, py) / wden;
    }
    const double eps = e[0] + e[1] * omega + e[2] * mu;
    Y.p1_table = (const float2 *)c->d_p1_table.ptr;
    Y.p1_eps = (float)e[0]; Y.p1_ew = (float)e[1]; Y.p1_em = (float)e[2];
    c->p1_eps_last = (float)eps;
    Y.p1_f = hrs ? p0.f[0] : p0.f[1]; Y.p1_c = hrs ? p0.c[0] : p0.c[1];
    // a single matrix: no first pass to certify (the table still serves the second); a certificate that would reject most pixels: the exact pass
    return p1_attach_audit(c, Y) && matrix_count > 1 && eps < 0.2;
}
// p1_setup for the radial models: the table over r, E = e0 + ew omega + em mu with the r form's coefficients.  With v = f c T(r) + c0, r = |(a, b)|, c = b (a):
//   |dv/dc| <= f (Tmax + r_max T1), |dv/d(other)| <= f r_max T1, so the two paths' errors in a, b (u D each: DESIGN.md section 2c, items 1-2) move v by at most
//   u G D, G = f (Tmax + 2 r_max T1);  the key — rho = fma(a, a, b b) (2u), the hardware's square root (1 ulp = 2u), the position's product (1u) — by 6 u f r_max^2 T1;
//   the table by f r_max e_table per path's share (chord of an interval h under T2, the entries' and the fma's roundings); the last two products and the fma 3 u vmag;
//   the EXACT path beyond its linear forms and divisions (in D): its r (2u), r_norm = k1 p (1u), the quotient, the product by pos, by f, the sum with c (5u vmag in
//   all) and the Newton result itself, f nu2 (p1_prepare_radial_gopro).
static int p1_setup_radial(gfw_ctx *c, const gfw_kernel_params &p0, const float *h_matrices, int matrix_count, double rho_max, ClipBatch *pending, GfwYuvArgs &Y, bool &fast1) {
    const bool hrs = (p0.flags & GFW_FLAG_HORIZONTAL_RS) != 0;
    double r_need = sqrt(rho_max);
    P1Radial *R = c->p1_radial;
    if (!(R && R->ok && R->model == c->model && memcmp(R->k, p0.k, sizeof(R->k)) == 0 && r_need <= R->r_max && r_need >= 0.7 * R->r_max)) {
        r_need = fmin(r_need * 1.08, 8.0);                       // head-room so that frame-to-frame motion does not rebuild the table
        if (!R) R = c->p1_radial = new P1Radial();
        std::vector<float2> tab;
        R->model = c->model;
        if (!p1_prepare_radial(c->model, p0, r_need, *R, &tab)) { R->ok = false; return GFW_OK; }
        { bool moved; const int rc = p1_table_upload(c, tab, pending, moved); if (rc != GFW_OK || !moved) { R->ok = false; return rc; } }
    }
    const double f = fabs((double)(hrs ? p0.f[0] : p0.f[1])), cc = fabs((double)(hrs ? p0.c[0] : p0.c[1]));
    const double rmax = R->r_max, vmag = f * rmax * R->Tmax + cc, u24 = 1.05 / 16777216.0;
    const double G = f * (R->Tmax + 2.0 * rmax * R->T1);
    const double e0 = u24 * (G * 10.0 * rmax + 6.0 * f * rmax * rmax * R->T1 + 11.0 * vmag) + 2.0 * f * rmax * R->etab + 1.05 * f * R->nu2 + 1.0 / 16384.0;
    const double e[3] = {e0, u24 * G * rmax, u24 * G};
    Y.p1_rho_max = (float)(rmax * rmax * (1.0 - 1e-6)); Y.p1_kmax = (float)rmax; Y.p1_rho_scale = (float)(GFW_P1_TABLE_N / rmax); Y.p1_rform = 1;
    Y.p1_lat[0] = (float)(R->Tmax * (1.0 + 1e-6)); Y.p1_lat[1] = (float)(0.5 * R->T1 * (1.0 + 1e-6)); Y.p1_lat[2] = (float)(0.5 * rmax * R->T1 * (1.0 + 1e-6));
    Y.p1_lat[3] = (float)(0.25 * (rmax * R->T2 + R->T1) * (1.0 + 1e-6)); Y.p1_lat[4] = (float)(4.0 * u24 * vmag + 1.0 / 131072.0);
    Y.p1_lat[5] = 1.0f;                                          // the per-pixel form (header comment of p1_prepare_radial_gopro)
    fast1 = p1_finish(c, p0, h_matrices, matrix_count, rmax, e, Y);      // (its audit is a specialised audit build: gfw_api_bake.inc)
    return GFW_OK;
}
// The half-extents of the output frame's corner ray in normalised camera coordinates (new_k = f / fov, frame_transform.rs:37-51; the zoom centre moves it by
// translation2d) — the first pass's range estimate for device-resident tables
static void p1_corner_extent(const gfw_kernel_params &p0, double &hx, double &hy) {
    hx = 0.5 * p0.output_width * (double)p0.fov / fmax(fabs((double)p0.f[0]), 1e-6) + fabs((double)p0.translation2d[0]) * (double)p0.fov / fmax(fabs((double)p0.f[0]), 1e-6);
    hy = 0.5 * p0.output_height * (double)p0.fov / fmax(fabs((double)p0.f[1]), 1e-6) + fabs((double)p0.translation2d[1]) * (double)p0.fov / fmax(fabs((double)p0.f[1]), 1e-6);
}
// Fill the first-pass fields of the fused kernel's arguments.  `fast1`: the certified pass may be used (false on every early return: the exact first pass).
static int p1_setup(gfw_ctx *c, const gfw_kernel_params &p0, const float *h_matrices, int matrix_count, ClipBatch *pending, GfwYuvArgs &Y, bool &fast1) {
    Y.p1_table = nullptr; Y.audit = nullptr; fast1 = false;
    if (c->kernel_variant == 2) return GFW_OK;                  // forced exact first pass (tests / A-B benchmarking)
    const bool radial = p1_model_radial_served(c->model);       // (round 6) GoPro, Sony, generic polynomial: certified through a table over r, in specialised builds only
    if ((c->model != GFW_MODEL_OPENCV_FISHEYE && !radial) || Y.hstretch_div || Y.vstretch_div) return GFW_OK;
    if (radial && c->jit_mode == 0) return GFW_OK;
    if (radial) {                                               // GFW_P1_RADIAL=0 in the environment: the exact first pass for these models (A/B runs)
        static const bool env_off = [] { const char *e = getenv("GFW_P1_RADIAL"); return e && e[0] == '0' && e[1] == 0; }();
        if (env_off) return GFW_OK;
    }
    const bool hrs = (p0.flags & GFW_FLAG_HORIZONTAL_RS) != 0;
    // rho range over the output frame under the mid-row matrix (corners + edge midpoints), in double
    double rho_max = 0.0;
    if (h_matrices) {
        const float *m = h_matrices + (size_t)(matrix_count >> 1) * 14;
        const double xs[3] = {0.0, p0.output_width * 0.5, (double)p0.output_width}, ys[3] = {0.0, p0.output_height * 0.5, (double)p0.output_height};
        for (double y : ys) for (double x : xs) {
            const double ox = x + p0.translation2d[0], oy = y + p0.translation2d[1];
            const double X = ox * m[0] + oy * m[1] + m[2], Yy = ox * m[3] + oy * m[4] + m[5], W = ox * m[6] + oy * m[7] + m[8];
            if (!(W > 0.05)) { rho_max = 1e9; continue; }
            rho_max = fmax(rho_max, (X * X + Yy * Yy) / (W * W));
        }
        rho_max = rho_max * 1.25 + 0.01;
    } else {
        // device-resident matrices: no host view of the geometry.  Bound the corner ray from the intrinsics
        // (new_k = f / fov, frame_transform.rs:37-51) and allow 15 degrees of stabilisation rotation on top (rays beyond it simply take the exact path).
        // (a launch of gfw_undistort_clip_params: the envelope of its frames — one table serves every frame of the call, built at most once)
        double hx, hy;
        p1_corner_extent(p0, hx, hy);
        clip_envelope(pending, hx, hy);
        const double ang = atan(sqrt(hx * hx + hy * hy)) + 0.26;
        rho_max = ang < 1.45 ? tan(ang) * tan(ang) : 64.0;
    }
    if (!(rho_max == rho_max)) return GFW_OK;
    if (rho_max > 64.0) rho_max = 64.0;
    if (radial) return p1_setup_radial(c, p0, h_matrices, matrix_count, rho_max, pending, Y, fast1);
    if (!(c->p1_valid && memcmp(c->p1_k, p0.k, sizeof(c->p1_k)) == 0 && rho_max <= c->p1_rho_max && rho_max >= 0.5 * c->p1_rho_max))
        rho_max = fmin(rho_max * 1.15, 64.0);                   // head-room so that frame-to-frame motion does not rebuild the table
    { bool ready; const int rc = p1_prepare_table(c, p0, (float)rho_max, pending, ready); if (rc != GFW_OK || !ready) return rc; }
    const double f = fabs((double)(hrs ? p0.f[0] : p0.f[1])), cc = fabs((double)(hrs ? p0.c[0] : p0.c[1]));
    const double rmax = sqrt((double)c->p1_rho_max);
    const double vmag = f * rmax * c->p1_smax + cc;
    // E >= |approx - exact| (DESIGN.md section 2c, derived operation by operation): with u = 2^-24,
    //   E = 1.05 u { G * (mu + rmax omega + 10 rmax) + 6 |f| rmax rho_max S' + |f| rmax smax (kappa + 4) + 2 vmag } + 2 |f| rmax e_table + 2^-14,
    //   G = |f| smax + 2 sqrt2 |f| rmax^2 S',   S' = max |ds/drho|,
    // mu and omega measure the rounding error of the mid-row matrix's linear forms relative to W (gfw_frame.hip: p1_bound): the kernel
    // evaluates them from the matrix it actually uses (device-resident tables included) and forms E = p1_eps + p1_ew * omega + p1_em * mu per frame.
    const double u24 = 1.05 / 16777216.0;
    const double G = f * c->p1_smax + 2.0 * M_SQRT2 * f * rmax * rmax * c->p1_slope;
    const double e0 = u24 * (G * 10.0 * rmax + 6.0 * f * rmax * (double)c->p1_rho_max * c->p1_slope + f * rmax * c->p1_smax * (c->p1_kappa + 4.0) + 2.0 * vmag)
                    + 2.0 * f * rmax * c->p1_etab + 1.0 / 16384.0;
    const double e[3] = {e0, u24 * G * rmax, u24 * G};
    Y.p1_rho_max = c->p1_rho_max; Y.p1_rho_scale = (float)(GFW_P1_TABLE_N / (double)c->p1_rho_max); Y.p1_kmax = c->p1_rho_max; Y.p1_rform = 0;
    // the lattice form of the first pass (gfw_frame.hip, phase 1): bounds on s and its derivatives for the curvature of v across a cell, and the roundings of the
    // interpolation itself (node differences, three fmas, the row fraction: < 4 u vmag; 2^-17 px on top)
    Y.p1_lat[0] = (float)(c->p1_smax * (1.0 + 1e-6)); Y.p1_lat[1] = (float)(c->p1_u1 * (1.0 + 1e-6)); Y.p1_lat[2] = (float)(c->p1_u2 * (1.0 + 1e-6));
    Y.p1_lat[3] = (float)(c->p1_t32 * (1.0 + 1e-6)); Y.p1_lat[4] = (float)(4.0 * u24 * vmag + 1.0 / 131072.0); Y.p1_lat[5] = 0.0f;
    {   // the per-pixel form of the first pass on request: GFW_OPT_KERNEL_VARIANT = 4 (audit of that form) or GFW_P1_LATTICE=0 in the environment (A/B runs)
        static const bool env_off = [] { const char *e = getenv("GFW_P1_LATTICE"); return e && e[0] == '0' && e[1] == 0; }();
        if (c->kernel_variant == 4 || env_off) Y.p1_lat[5] = 1.0f;
    }
    fast1 = p1_finish(c, p0, h_matrices, matrix_count, rmax, e, Y);
    return GFW_OK;
}

