// env_fit.inc -- the SPA envelope of an interval record as polynomials in w = t - t_j, shared by
// the preparation kernel k_items (emrifd_prepare.hip, EFD_HD = __device__) and the host twin
// (emrifd_cpu.cpp, EFD_HD empty). Both define TWO_PI, KTH0, the KRH / KTHN tables and
// env_rsqrt first.
//
// On one record the SPA term of a bin is (notebook Tutorial_FD_construction_single_mode.ipynb
// :599-616, uniform K_{1/3} form)
//     X(w) A(w) exp(i (2 pi g t - Phi(w) + theta(w) + sgn(F') 3 pi / 4)),
//     A(w) = rho(y) / sqrt|F'(w)|,   rho e^{i theta} = K_{1/3} factor / Q_spa,
//     y = 2 pi F'^3 / (3 F''^2)
// with rho and theta the polar series of the Hankel expansion (KRH, KTHN; |y| >= 153, where its
// four terms are exact to 1e-17). The straight-line evaluation spends 16 FP64 operations per bin
// on A and theta: F' and F'' quadratics, 1/sqrt|F'| with a Newton step, 1/|y| and the angle. Both
// are smooth on a record whose |y| stays large, so a record that passes the check below carries
// them as polynomials in w instead:
//   - A(w) of degree ENV_DEG = 6, interpolated at the Chebyshev nodes of [0, dtj]: 6 FMAs per bin;
//   - theta(w) as a cubic (the Chebyshev series from the same 7 nodes, truncated), folded into
//     the record's phase cubic (Phi - theta is still a cubic in w): no operation per bin. The
//     fold rounds Phi's constant term once more (half an ulp of |Phi(t_j)|, the size of the
//     rounding Phi(t_j) itself carries).
// The check evaluates both polynomials exactly as the kernel does (Horner in w) against the
// exact envelope at the 8 extrema of T_7 on [0, dtj] (where the interpolant's error peaks; 15
// envelope evaluations a record in all) and accepts the record when the error is at most
// ENV_TOL_A of max A (relative) and ENV_TOL_T
// rad (absolute): 1e-11 and 1e-10 of a term, 100x and 10x below the ~1e-9 rad rounding every
// term's phase carries at |Phi| ~ 1e7 (and 1e-8 at the higher harmonics' 1e8). Config 2: ~96% of
// the SPA evaluations (offline study, DESIGN.md Round 6; 91% with theta held to 1e-11).

constexpr int ENV_DEG = 6;
constexpr double ENV_TOL_A = 1e-11;
constexpr double ENV_TOL_T = 1e-10;
constexpr double ENV_MIN_Y = 153.0;   // |y| bound (with k_items' 10% margin) of the polar series

struct EnvFit {
    double a[ENV_DEG + 1];   // A(w), highest power first (Horner order)
    double th[4];            // theta(w), highest power first (the phase cubic's PPoly order)
};

// the exact envelope at w: F' = (fd0 w + fd1) w + fd2, F'' = (g0 w + g1) w + g2 (unscaled).
// env_rsqrt (defined by the includer: the hardware estimate with Newton steps on the device,
// 1 / sqrt on the host) gives 1/sqrt|F'|, whose square and cube make 1/|y| without a division.
EFD_HD inline void env_exact(const double* fd, const double* g, double thsign, double w, double& A,
                             double& th) {
    const double fdv = fma(fma(fd[0], w, fd[1]), w, fd[2]);
    const double fddv = fma(fma(g[0], w, g[1]), w, g[2]);
    const double r = env_rsqrt(fabs(fdv));                  // |F'|^-1/2
    const double r2 = r * r;
    const double wv = (3.0 / TWO_PI) * (fddv * fddv) * (r2 * r2 * r2);   // 1 / |y|
    const double u = wv * wv;
    const double rho = fma(fma(fma(KRH[3], u, KRH[2]), u, KRH[1]), u, KRH[0]);
    const double thn = wv * fma(fma(fma(KTHN[3], u, KTHN[2]), u, KTHN[1]), u, KTHN[0]);
    A = rho * r;
    th = thsign * thn;
}

// The interpolant's coefficients as fixed linear maps of the node values: with the nodes
// s_k = (1 + x_k) / 2 on [0, 1] (x_k = cos((2k + 1) pi / 14), the order of X7 below), the degree-6
// interpolant is sum_i p_i s^i with p = V^-1 f (V the nodes' Vandermonde matrix), and theta's
// cubic is the same Chebyshev series truncated after T_3, in powers of s (rows of ENV_W3). Both
// matrices are exact to 20 digits (40-digit arithmetic, DESIGN.md Round 6); as straight FMA rows
// they replace the DCT / Chebyshev-to-monomial recurrences' dependent loops.
constexpr double ENV_W7[7][7] = {
    {0.016096134271444435671, -0.049987876278138952482, 0.089763092195316248359,
     -0.14285714285714285714, 0.22735584042603871817, -0.40826225846748290607,
     1.2678922107099653135},
    {-1.5611206808249638003, 4.8427034533670126003, -8.6715802871824189021,
     13.714285714285714286, -21.477659819961722759, 36.267069138093393687,
     -23.113697517777015111},
    {23.657799130980610997, -72.945343029628708004, 128.65329371076214365,
     -196.57142857142857143, 280.6167526836103667, -307.68681980126998377,
     144.27574587697414186},
    {-127.47429180703558856, 388.40912535694742, -665.04385608430818017,
     950.85714285714285714, -1147.5887516125224832, 1020.2968632400355913,
     -419.45623195025961646},
    {303.57148687813961718, -907.70794227038331262, 1485.2199536674384576,
     -1938.2857142857142857, 2057.0738379869116891, -1620.7980723233742938,
     620.92645034698212816},
    {-327.1486125141159835, 951.87378616656146421, -1467.2157158196662427,
     1755.4285714285714286, -1695.9572695474555353, 1237.1098381877578567,
     -454.0905979016529879},
    {130.20653506929482857, -364.83060405905322015, 527.19549756118696301,
     -585.14285714285714286, 527.19549756118696301, -364.83060405905322015,
     130.20653506929482857}};
constexpr double ENV_W3[4][7] = {
    {-0.10165443621355265414, 0.10702091160166934744, 0.11930124891586627315,
     -0.14285714285714285714, -0.18986684997799971916, 0.30584819351622459786,
     0.90220807501493501199},
    {2.5185918758768087888, -2.2932605173801433673, -3.3408618646193829832,
     2.2857142857142857143, 6.1911009588307362656, 1.2760219621512775191,
     -6.6373067005735819373},
    {-8.6629029186417365166, 6.4590248426552300049, 11.945320391387904255,
     -2.2857142857142857143, -14.795559485599257537, -5.4417862874263641567,
     12.781617743338509665},
    {7.1481735539934153939, -3.9669370433605313872, -8.9136266256623872642, 0.0,
     8.9136266256623872642, 3.9669370433605313872, -7.1481735539934153939}};

// out[R - 1 - i] = (sum_k M[i][k] f[k]) / dtj^i: row i of M applied to the node values, as the
// coefficient of w^i (highest power first)
template <int R>
EFD_HD inline void env_apply(const double (*M)[7], const double* f, double dtj, double* out) {
    const double r = 1.0 / dtj;
    double rk = 1.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        double p = M[i][0] * f[0];
#pragma unroll
        for (int k = 1; k < 7; ++k) p = fma(M[i][k], f[k], p);
        out[R - 1 - i] = p * rk;
        rk *= r;
    }
}

// The record's envelope polynomials, or false when they miss the tolerances (or meet a
// non-finite value). fd: F' quadratic; g: F'' quadratic (unscaled); fdneg: F' < 0 on the record.
EFD_HD inline bool env_fit(const double* fd, const double* g, double dtj, bool fdneg, EnvFit& E) {
    constexpr double X7[7] = {0.97492791218182360702, 0.78183148246802980871,
                              0.43388373911755812048, 0.0, -0.43388373911755812048,
                              -0.78183148246802980871, -0.97492791218182360702};
    // check points s = w / dtj: the extrema of T_7 on [0, 1], where the interpolant's error
    // (~ c_7 T_7) peaks, both ends included
    constexpr double SC[8] = {0.0, 0.049515566048790436882, 0.18825509907063323474,
                              0.38873953302184279786, 0.61126046697815720214,
                              0.81174490092936676526, 0.95048443395120956312, 1.0};
    const double thsign = fdneg ? -KTH0 : KTH0;
    double fa[7], ft[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) env_exact(fd, g, thsign, dtj * fma(0.5, X7[k], 0.5), fa[k], ft[k]);
    env_apply<ENV_DEG + 1>(ENV_W7, fa, dtj, E.a);
    env_apply<4>(ENV_W3, ft, dtj, E.th);   // theta: the series truncated to a cubic
    double amax = 0.0, ea = 0.0, et = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double w = dtj * SC[k];
        double A, th;
        env_exact(fd, g, thsign, w, A, th);
        double pa = E.a[0];
        for (int i = 1; i <= ENV_DEG; ++i) pa = fma(pa, w, E.a[i]);
        const double pt = fma(fma(fma(E.th[0], w, E.th[1]), w, E.th[2]), w, E.th[3]);
        amax = fmax(amax, fabs(A));
        ea = fmax(ea, fabs(pa - A));
        et = fmax(et, fabs(pt - th));
        if (!(fabs(A) < INFINITY && fabs(pa) < INFINITY && fabs(pt) < INFINITY)) return false;
    }
    return ea <= ENV_TOL_A * amax && et <= ENV_TOL_T;
}
