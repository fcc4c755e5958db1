/*
 * cp_oracle.c — CPU restatement of the batched cartpole++ hot path.
 * TEST INFRASTRUCTURE ONLY (see cp_oracle.h): the parity oracle for the HIP
 * kernel and the CPU baseline of bench.py.  Never linked by the product.
 *
 * Control flow follows the reference env:
 *   reset  bullet_cartpole.py:313-346 (+ bump_cart :348-352, random_force_in_plane :354-359)
 *   step   bullet_cartpole.py:178-275 (force applied AFTER each substep :199-207)
 *   obs    bullet_cartpole.py:298-311 (+ state_fields_of_pose_of :43-45)
 * Physics restates the Bullet step the scene exercises (SURVEY.md §8a rows a8-a10,
 * all [ext]; parity vs pybullet is UNPINNED) — the exact model is DESIGN.md
 * §Physics model.  Scene constants come from models/{ground,cart,pole,cart2,pole2}.urdf.
 *
 * Numerics: every multiply-add that the HIP kernel fuses is written here as an
 * explicit fma, the file is compiled with -ffp-contract=off, and the few
 * transcendentals are own polynomials, so the fp32 build reproduces the kernel
 * bit for bit.  ORC_DOUBLE builds the same algorithm in fp64.
 */
#include "cp_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#if defined(ORC_DEBUG) || defined(ORC_STATS)
#include <stdio.h>
#endif
#ifdef _OPENMP
#include <omp.h>
#endif

#ifdef ORC_DOUBLE
typedef double real;
#define FMA fma
#define SQRT sqrt
#define FABS fabs
#else
typedef float real;
#define FMA fmaf
#define SQRT sqrtf
#define FABS fabsf
#endif
#define RC(x) ((real)(x))

int orc_sizeof_real(void) { return (int)sizeof(real); }

/* ------------------------------------------------------------------ vectors */
typedef struct { real x, y, z; } v3;

static inline v3 mk(real x, real y, real z) { v3 r = {x, y, z}; return r; }
static inline v3 add(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 scl(v3 a, real s) { return mk(a.x * s, a.y * s, a.z * s); }
static inline v3 neg(v3 a) { return mk(-a.x, -a.y, -a.z); }
/* a + b*s */
static inline v3 madd(v3 a, v3 b, real s) { return mk(FMA(b.x, s, a.x), FMA(b.y, s, a.y), FMA(b.z, s, a.z)); }
static inline real dot(v3 a, v3 b) { return FMA(a.x, b.x, FMA(a.y, b.y, a.z * b.z)); }
static inline v3 cross(v3 a, v3 b) {
    return mk(FMA(a.y, b.z, -(a.z * b.y)), FMA(a.z, b.x, -(a.x * b.z)), FMA(a.x, b.y, -(a.y * b.x)));
}
static inline real comp(v3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

/* box axes from a unit quaternion (x,y,z,w): ax[i] = world direction of local axis i */
static void quat_axes(const real q[4], v3 ax[3]) {
    real x = q[0], y = q[1], z = q[2], w = q[3];
    real x2 = x + x, y2 = y + y, z2 = z + z;
    real xx = x * x2, yy = y * y2, zz = z * z2;
    real xy = x * y2, xz = x * z2, yz = y * z2;
    real wx = w * x2, wy = w * y2, wz = w * z2;
    ax[0] = mk(RC(1) - (yy + zz), xy + wz, xz - wy);
    ax[1] = mk(xy - wz, RC(1) - (xx + zz), yz + wx);
    ax[2] = mk(xz + wy, yz - wx, RC(1) - (xx + yy));
}
/* local -> world: ax0*l.x + ax1*l.y + ax2*l.z */
static inline v3 rot(const v3 ax[3], v3 l) {
    return mk(FMA(ax[0].x, l.x, FMA(ax[1].x, l.y, ax[2].x * l.z)),
              FMA(ax[0].y, l.x, FMA(ax[1].y, l.y, ax[2].y * l.z)),
              FMA(ax[0].z, l.x, FMA(ax[1].z, l.y, ax[2].z * l.z)));
}
static inline v3 rot_t(const v3 ax[3], v3 w) { return mk(dot(ax[0], w), dot(ax[1], w), dot(ax[2], w)); }

/* world inverse inertia M = sum_k iI[k] ax_k ax_k^T, stored xx xy xz yy yz zz */
static void world_inv_inertia(const v3 ax[3], const float iI[3], real M[6]) {
    v3 t0 = scl(ax[0], (real)iI[0]), t1 = scl(ax[1], (real)iI[1]), t2 = scl(ax[2], (real)iI[2]);
    M[0] = FMA(t0.x, ax[0].x, FMA(t1.x, ax[1].x, t2.x * ax[2].x));
    M[1] = FMA(t0.x, ax[0].y, FMA(t1.x, ax[1].y, t2.x * ax[2].y));
    M[2] = FMA(t0.x, ax[0].z, FMA(t1.x, ax[1].z, t2.x * ax[2].z));
    M[3] = FMA(t0.y, ax[0].y, FMA(t1.y, ax[1].y, t2.y * ax[2].y));
    M[4] = FMA(t0.y, ax[0].z, FMA(t1.y, ax[1].z, t2.y * ax[2].z));
    M[5] = FMA(t0.z, ax[0].z, FMA(t1.z, ax[1].z, t2.z * ax[2].z));
}
static inline v3 symv(const real M[6], v3 v) {
    return mk(FMA(M[0], v.x, FMA(M[1], v.y, M[2] * v.z)),
              FMA(M[1], v.x, FMA(M[3], v.y, M[4] * v.z)),
              FMA(M[2], v.x, FMA(M[4], v.y, M[5] * v.z)));
}

/* --------------------------------------------------------- own transcendentals */
#ifdef ORC_DOUBLE
/* fp64: the Taylor series through x^17 / x^18 (remainder < 1e-19 at pi/4): double-accurate */
static const double SIN64[8] = {-0.16666666666666666, 0.008333333333333333, -0.0001984126984126984,
                                2.7557319223985893e-06, -2.505210838544172e-08, 1.6059043836821613e-10,
                                -7.647163731819816e-13, 2.8114572543455206e-15};
static const double COS64[9] = {-0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05,
                                -2.755731922398589e-07, 2.08767569878681e-09, -1.1470745597729725e-11,
                                4.779477332387385e-14, -1.5619206968586225e-16};
#endif
static inline void sincos_small(real x, real* s, real* c) {
#ifdef ORC_DOUBLE
    real x2 = x * x, p = SIN64[7], q = COS64[8];
    for (int k = 6; k >= 0; --k) p = FMA(x2, p, SIN64[k]);
    *s = FMA(x * x2, p, x);
    for (int k = 7; k >= 0; --k) q = FMA(x2, q, COS64[k]);
    *c = FMA(x2, q, RC(1.0));
#else
    /* Taylor through x^9 / x^8; used for |x| <= pi/4 (fp32: below the format's rounding) */
    real x2 = x * x;
    real p = FMA(x2, RC(2.7557319223985893e-6), RC(-1.9841269841269841e-4));
    p = FMA(x2, p, RC(8.3333333333333333e-3));
    p = FMA(x2, p, RC(-1.6666666666666667e-1));
    *s = FMA(x * x2, p, x);
    real q = FMA(x2, RC(2.4801587301587302e-5), RC(-1.3888888888888889e-3));
    q = FMA(x2, q, RC(4.1666666666666667e-2));
    q = FMA(x2, q, RC(-0.5));
    *c = FMA(x2, q, RC(1.0));
#endif
}

/* sin/cos of 2*pi*u for u in [0,1) (bump direction, bullet_cartpole.py:355) */
static void sincos_turns(real u, real* s_out, real* c_out) {
    real y = u * RC(4.0);
    int q = (int)y;
    if (q > 3) q = 3;
    real f = y - (real)q;
    real x = (f - RC(0.5)) * RC(1.5707963267948966);
    real s, c;
    sincos_small(x, &s, &c);
    real S = (s + c) * RC(0.7071067811865476);
    real C = (c - s) * RC(0.7071067811865476);
    switch (q) {
        case 0: *s_out = S; *c_out = C; break;
        case 1: *s_out = C; *c_out = -S; break;
        case 2: *s_out = -S; *c_out = -C; break;
        default: *s_out = -C; *c_out = S; break;
    }
}
void orc_sincos_turns(float u, float* s, float* c) {
    real rs, rc;
    sincos_turns((real)u, &rs, &rc);
    *s = (float)rs;
    *c = (float)rc;
}

/* atan on [0, inf) (Cephes-style reduction + polynomial) */
static real atan_pos(real z) {
    real base = RC(0);
    if (z > RC(2.414213562373095)) {
        base = RC(1.5707963267948966);
        z = RC(-1.0) / z;
    } else if (z > RC(0.4142135623730950)) {
        base = RC(0.7853981633974483);
        z = (z - RC(1.0)) / (z + RC(1.0));
    }
    real z2 = z * z;
#ifdef ORC_DOUBLE
    {   /* fp64: odd Taylor series through z^47 on |z| <= tan(pi/8) (remainder < 1e-18) */
        real p = -1.0 / 47.0;
        for (int k = 22; k >= 1; --k) p = FMA(z2, p, (k & 1 ? -1.0 : 1.0) / (double)(2 * k + 1));
        return base + FMA(z * z2, p, z);
    }
#endif
    real p = FMA(z2, RC(8.05374449538e-2), RC(-1.38776856032e-1));
    p = FMA(z2, p, RC(1.99777106478e-1));
    p = FMA(z2, p, RC(-3.33329491539e-1));
    return base + FMA(z * z2, p, z);
}
static real atan2_own(real y, real x) {
    if (x == RC(0) && y == RC(0)) return RC(0);
    real ax = FABS(x), ay = FABS(y);
    real r = (ay <= ax) ? atan_pos(ay / ax) : RC(1.5707963267948966) - atan_pos(ax / ay);
    if (x < RC(0)) r = RC(3.141592653589793) - r;
    if (y < RC(0)) r = -r;
    return r;
}
/* test probe of the own transcendentals in the build's real type: sin, cos of x (|x| <= pi/4),
   atan2(y, x), sin, cos of 2 pi u (u in [0, 1)) */
void orc_probe_transcendentals(double x, double y, double u, double out[5]) {
    real s, c;
    sincos_small((real)x, &s, &c);
    out[0] = (double)s;
    out[1] = (double)c;
    out[2] = (double)atan2_own((real)y, (real)x);
    sincos_turns((real)u, &s, &c);
    out[3] = (double)s;
    out[4] = (double)c;
}

/* pybullet getEulerFromQuaternion (roll, pitch, yaw) [ext: recalled formula] */
static void quat_euler(const real q[4], real rpy[3]) {
    real x = q[0], y = q[1], z = q[2], w = q[3];
    real sqw = w * w, sqx = x * x, sqy = y * y, sqz = z * z;
    rpy[0] = atan2_own(RC(2) * FMA(y, z, w * x), ((sqw - sqx) - sqy) + sqz);
    real sarg = RC(-2) * FMA(x, z, -(w * y));
    if (sarg <= RC(-1)) rpy[1] = RC(-1.5707963267948966);
    else if (sarg >= RC(1)) rpy[1] = RC(1.5707963267948966);
    else rpy[1] = atan2_own(sarg, SQRT(FMA(-sarg, sarg, RC(1))));
    rpy[2] = atan2_own(RC(2) * FMA(x, y, w * z), ((sqw + sqx) - sqy) - sqz);
}

/* ------------------------------------------------------------------ Philox */

/* --------------------------------------------------------------- raster obs */
/* Restatement of the kernel's ray caster (cartpoleplusplus_amd/csrc/cp_raster.h),
 * which stands in for bullet_cartpole.py:277-296 (render_rgb: TinyRenderer through
 * p.renderImage, not available here).  Same fp32 operations in the same order. */
static int raster_u8(real x) {
    x = x > RC(1) ? RC(1) : (x < RC(0) ? RC(0) : x);
    return (int)(x * RC(255) + RC(0.5));
}
static int ray_box(v3 eye, v3 d, v3 cc, const v3 ax[3], const real h[3], real* t, int* axis, real* sgn) {
    v3 oc = sub(eye, cc);
    real lo[3], hi[3], dd[3];
    for (int i = 0; i < 3; ++i) {
        real o = dot(oc, ax[i]);
        dd[i] = dot(d, ax[i]);
        real inv = RC(1) / dd[i];
        real t1 = (-h[i] - o) * inv, t2 = (h[i] - o) * inv;
        int lt = t1 < t2;
        lo[i] = lt ? t1 : t2;
        hi[i] = lt ? t2 : t1;
    }
    real tmin = lo[0];
    int a = 0;
    if (lo[1] > tmin) { tmin = lo[1]; a = 1; }
    if (lo[2] > tmin) { tmin = lo[2]; a = 2; }
    real tmax = hi[0] < hi[1] ? hi[0] : hi[1];
    tmax = tmax < hi[2] ? tmax : hi[2];
    *t = tmin;
    *axis = a;
    *sgn = dd[a] > RC(0) ? RC(-1) : RC(1);
    return tmin <= tmax && tmin > RC(0);
}
/* One frame of camera `cam` for the body poses pose[d] = (xyz, quat xyzw) of
 * cart, pole, cart2, pole2: rgb uint8 [H][W][3]. */
void orc_render_frame(const cp_raster_config* rc, const cp_physics* P, const float pose[4][7], int cam,
                      uint8_t* rgb) {
    const int W = rc->width, H = rc->height;
    v3 eye = mk((real)rc->eye[cam][0], (real)rc->eye[cam][1], (real)rc->eye[cam][2]);
    v3 F = sub(mk((real)rc->target[0], (real)rc->target[1], (real)rc->target[2]), eye);
    real lf = SQRT(dot(F, F));
    v3 f = mk(F.x / lf, F.y / lf, F.z / lf);
    v3 rr = cross(f, mk((real)rc->up[0], (real)rc->up[1], (real)rc->up[2]));
    real lr = SQRT(dot(rr, rr));
    v3 r = mk(rr.x / lr, rr.y / lr, rr.z / lr);
    v3 u = cross(r, f);
    const real syk = (real)rc->tan_half_fov;
    const real sxk = (real)rc->tan_half_fov * ((real)W / (real)H);
    v3 bc[CP_NUM_BODIES], bax[CP_NUM_BODIES][3];
    real bh[CP_NUM_BODIES][3];
    bc[0] = mk(RC(0), RC(0), RC(0));
    bax[0][0] = mk(RC(1), RC(0), RC(0)); bax[0][1] = mk(RC(0), RC(1), RC(0)); bax[0][2] = mk(RC(0), RC(0), RC(1));
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        real q[4] = {pose[d][3], pose[d][4], pose[d][5], pose[d][6]};
        bc[d + 1] = mk(pose[d][0], pose[d][1], pose[d][2]);
        quat_axes(q, bax[d + 1]);
    }
    for (int b = 0; b < CP_NUM_BODIES; ++b)
        for (int k = 0; k < 3; ++k) bh[b][k] = (real)P->half_extents[b][k];
    v3 light = mk((real)rc->light[0], (real)rc->light[1], (real)rc->light[2]);
    for (int py = 0; py < H; ++py) {
        for (int px = 0; px < W; ++px) {
            real sx = ((RC(2) * ((real)px + RC(0.5))) / (real)W - RC(1)) * sxk;
            real sy = (RC(1) - (RC(2) * ((real)py + RC(0.5))) / (real)H) * syk;
            v3 d = mk(FMA(sy, u.x, FMA(sx, r.x, f.x)), FMA(sy, u.y, FMA(sx, r.y, f.y)), FMA(sy, u.z, FMA(sx, r.z, f.z)));
            real best = (real)rc->far_plane;
            int hit = -1;
            v3 n = mk(RC(0), RC(0), RC(1));
            for (int b = 0; b < CP_NUM_BODIES; ++b) {
                real t, sg;
                int ax;
                if (ray_box(eye, d, bc[b], bax[b], bh[b], &t, &ax, &sg) && t < best) {
                    best = t;
                    hit = b;
                    n = scl(bax[b][ax], sg);
                }
            }
            uint8_t* o = rgb + ((size_t)py * W + px) * 3;
            if (hit < 0) {
                for (int c = 0; c < 3; ++c) o[c] = (uint8_t)raster_u8((real)rc->background[c]);
                continue;
            }
            real ndl = dot(n, light);
            real sh = FMA((real)rc->diffuse, ndl > RC(0) ? ndl : RC(0), (real)rc->ambient);
            for (int c = 0; c < 3; ++c) o[c] = (uint8_t)raster_u8((real)rc->color[hit][c] * sh);
        }
    }
}

void orc_philox4x32_10(const uint32_t ctr_in[4], const uint32_t key_in[2], uint32_t out[4]) {
    uint32_t c0 = ctr_in[0], c1 = ctr_in[1], c2 = ctr_in[2], c3 = ctr_in[3];
    uint32_t k0 = key_in[0], k1 = key_in[1];
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* ------------------------------------------------------------ scene / config */
void orc_default_config(cp_config* c) {
    memset(c, 0, sizeof(*c));
    c->num_envs = 1;
    c->action_repeats = 2;           /* bullet_cartpole.py:23 */
    c->steps_per_repeat = 1;         /* :25 */
    c->max_episode_len = 200;        /* :31 */
    c->action_force = 50.0f;         /* :18 */
    c->initial_force = 200.0f;       /* :20 */
    c->random_theta = 1;             /* :22 */
    c->initial_force_steps = 30;     /* :76 */
    c->settle_steps = 100;           /* :326 */
    c->done_on_bounds = 0;
    c->pos_threshold = 3.0f;         /* :58 */
    c->angle_threshold = 0.35f;      /* :62 */
    c->tan_angle_threshold = (float)tan(0.35f);
    c->sin_angle_threshold = (float)sin(0.35f);
    c->autoreset = 0;
    c->bump_mode = CP_BUMP_PHILOX;
    c->seed = 0;
    c->env_id_offset = 0;
    cp_physics* p = &c->phys;
    p->dt = (float)(1.0 / 240.0);
    p->inv_dt = (float)240.0;
    p->gravity[0] = 0.0f; p->gravity[1] = 0.0f; p->gravity[2] = -9.81f;  /* :152 */
    p->lin_damping = 0.04f;
    p->ang_damping = 0.04f;
    p->erp = 0.2f;
    p->contact_margin = 0.02f;
    p->residual_threshold = 1e-7f;
    p->solver_iterations = 50;
    p->edge_bias = 1e-4f;
    p->max_angular_step = (float)(0.25 * 3.141592653589793);
    p->warmstart = 0.85f;
    p->max_coord_velocity = 100.0f;   /* btMultiBody m_maxCoordinateVelocity [ext] */
    p->sleep_epsilon = 0.05f;         /* btMultiBody SLEEP_EPSILON [ext] (CP_MODEL_SLEEPING) */
    p->sleep_timeout = 2.0f;          /* btMultiBody SLEEP_TIMEOUT [ext] */
    /* models/ground.urdf: static box 3 x 3 x 0.1, no <contact> -> default friction 0.5 */
    const double he[5][3] = {{1.5, 1.5, 0.05}, {0.1, 0.1, 0.025}, {0.005, 0.005, 0.25},
                             {0.1, 0.1, 0.025}, {0.005, 0.005, 0.25}};
    const double mass[5] = {0.0, 1.0, 5.0, 1.0, 5.0};
    const double inert[5][3] = {{0, 0, 0},
                                {0.0035416666666, 0.0035416666666, 0.0066666666666},
                                {0.104208333333333, 0.104208333333333, 0.00008333333333},
                                {0.0035416666666, 0.0035416666666, 0.0066666666666},
                                {0.104208333333333, 0.104208333333333, 0.00008333333333}};
    const double mu[5] = {0.5, 0.0, 1.0, 0.0, 1.0};
    const double spawn[5][3] = {{0, 0, 0}, {0, 0, 0.08}, {0, 0, 0.35}, {1, 0, 0.08}, {1, 0, 0.35}};
    for (int b = 0; b < 5; ++b) {
        for (int k = 0; k < 3; ++k) {
            p->half_extents[b][k] = (float)he[b][k];
            p->inertia[b][k] = (float)inert[b][k];
            p->inv_inertia[b][k] = inert[b][k] > 0 ? (float)(1.0 / inert[b][k]) : 0.0f;
            p->spawn_pos[b][k] = (float)spawn[b][k];
        }
        p->inv_mass[b] = mass[b] > 0 ? (float)(1.0 / mass[b]) : 0.0f;
        p->friction[b] = (float)mu[b];
    }
}

static const int PAIR_A[CP_NUM_PAIRS] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
static const int PAIR_B[CP_NUM_PAIRS] = {1, 2, 3, 4, 2, 3, 4, 3, 4, 4};
/* Contact islands: island 0 = {ground, cart, pole} (pairs 0, 1, 4), island 1 =
 * {ground, cart2, pole2} (pairs 2, 3, 9); the cross pairs 5, 6 (cart-cart2, cart-pole2)
 * are stored with island 0 and 7, 8 (pole-cart2, pole-pole2) with island 1.  Merged
 * solve order over pairs: 0 2 1 3 4 9 5 6 7 8 (rows of different islands share no
 * dynamic body, so the kernel runs the two islands' rows side by side).
 * island p's local pairs j = 0..4 -> global pair (own 3, then the 2 cross pairs it stores) */
static const int ISLAND_PAIR[CP_NUM_ISLANDS][CP_ISLAND_PAIRS] = {{0, 1, 4, 5, 6}, {2, 3, 9, 7, 8}};

/* --------------------------------------------------------------- simulation */
/* CP_MODEL_PERSISTENT: one pair's persistent contact manifold, Bullet's btPersistentManifold
 * restated (oracle only): up to 4 cached points, each with its local points on A and B
 * (m_localPointA/B), its normal (stored A -> B here; Bullet keeps m_normalWorldOnB = -n), its
 * separation m_distance1 and its applied normal impulse (the warm start). */
typedef struct { int cnt; v3 la[4], lb[4], n[4]; real d[4], lam[4]; } pman_t;

typedef struct {
    v3 x[CP_NUM_DYN];
    real q[CP_NUM_DYN][4];
    v3 v[CP_NUM_DYN], w[CP_NUM_DYN];
    v3 f[CP_NUM_DYN];          /* pending world force */
    v3 ax[CP_NUM_DYN][3];
    real M[CP_NUM_DYN][6];
    uint32_t ws_id[CP_NUM_ISLANDS][CP_ISLAND_PAIRS];   /* warm-start cache (4 packed feature ids) */
    real ws_lam[CP_NUM_ISLANDS][CP_ISLAND_PAIRS][4];
    pman_t pm[CP_NUM_ISLANDS][CP_ISLAND_PAIRS];        /* CP_MODEL_PERSISTENT only */
    int32_t slp_a[CP_NUM_DYN];  /* CP_MODEL_SLEEPING: activation word (CP_ACT_* | CP_ACT_AWAKE) */
    real slp_t[CP_NUM_DYN];     /*                    btMultiBody::m_sleepTimer */
} sim_t;

typedef struct { v3 n; int cnt, base, fcnt, fbase; real mu; } manifold_t;
/* n: the row's normal (the manifold normal, or a cached point's own normal under
 * CP_MODEL_PERSISTENT); pm: index of the cached point (CP_MODEL_PERSISTENT) */
typedef struct { v3 rb, n; real inv_eff, target, lam; int id, pm; } point_t;
/* t1, t2: the friction directions (btPlaneSpace1 of the normal, or velocity-dependent) */
typedef struct { real lam1, lam2, inv_eff1, inv_eff2; v3 t1, t2; } fpoint_t;

/* collision shape accessor: body g (0 = ground, static at the origin, identity axes) */
typedef struct { v3 c; v3 ax[3]; real h[3]; } box_t;

static void get_box(const sim_t* S, const cp_physics* P, int g, box_t* b) {
    for (int k = 0; k < 3; ++k) b->h[k] = (real)P->half_extents[g][k];
    if (g == 0) {
        b->c = mk(RC(0), RC(0), RC(0));
        b->ax[0] = mk(RC(1), RC(0), RC(0));
        b->ax[1] = mk(RC(0), RC(1), RC(0));
        b->ax[2] = mk(RC(0), RC(0), RC(1));
    } else {
        b->c = S->x[g - 1];
        for (int k = 0; k < 3; ++k) b->ax[k] = S->ax[g - 1][k];
    }
}

typedef struct { real u, v, n; int id; } cand_t;

/* Face contact: reference face (axis ri, outward normal nr) of box R against the
 * most anti-parallel face of box I.  Candidate points, in canonical order:
 *   C1 incident face vertices inside the reference rectangle,
 *   C2 reference rectangle corners strictly inside the incident face,
 *   C3 incident-edge x rectangle-side crossings.
 * Keep depth <= margin; reduce > 4 to 4 (deepest, farthest, max/min area). */
static int face_contact(const box_t* R, int ri, v3 nr, const box_t* I, real margin,
                        v3 pts[4], real dist[4], int fid[4]) {
    int r1 = (ri + 1) % 3, r2 = (ri + 2) % 3;
    v3 fc = madd(R->c, nr, R->h[ri]);
    v3 u = R->ax[r1], v = R->ax[r2];
    real hu = R->h[r1], hv = R->h[r2];
    /* incident face */
    real e0 = dot(nr, I->ax[0]), e1d = dot(nr, I->ax[1]), e2d = dot(nr, I->ax[2]);
    int j = 0;
    real best = FABS(e0);
    if (FABS(e1d) > best) { j = 1; best = FABS(e1d); }
    if (FABS(e2d) > best) { j = 2; }
    real ej = (j == 0) ? e0 : (j == 1 ? e1d : e2d);
    real isg = (ej > RC(0)) ? RC(-1) : RC(1);
    v3 ic = madd(I->c, I->ax[j], isg * I->h[j]);
    int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    v3 E1 = scl(I->ax[j1], I->h[j1]);
    v3 E2 = scl(I->ax[j2], I->h[j2]);
    v3 icr = sub(ic, fc);
    real cu = dot(icr, u), cv = dot(icr, v), cn = dot(icr, nr);
    real e1u = dot(E1, u), e1v = dot(E1, v), e1n = dot(E1, nr);
    real e2u = dot(E2, u), e2v = dot(E2, v), e2n = dot(E2, nr);

    cand_t P[4];
    P[0].id = 0; P[1].id = 1; P[2].id = 2; P[3].id = 3;
    P[0].u = (cu + e1u) + e2u; P[0].v = (cv + e1v) + e2v; P[0].n = (cn + e1n) + e2n;
    P[1].u = (cu - e1u) + e2u; P[1].v = (cv - e1v) + e2v; P[1].n = (cn - e1n) + e2n;
    P[2].u = (cu - e1u) - e2u; P[2].v = (cv - e1v) - e2v; P[2].n = (cn - e1n) - e2n;
    P[3].u = (cu + e1u) - e2u; P[3].v = (cv + e1v) - e2v; P[3].n = (cn + e1n) - e2n;

    cand_t cand[24];
    int nc = 0;
    /* C1 */
    int inside = 0;
    for (int k = 0; k < 4; ++k) {
        int in = FABS(P[k].u) <= hu && FABS(P[k].v) <= hv;
        inside += in;
        if (in && P[k].n <= margin) cand[nc++] = P[k];
    }
    /* all four incident vertices inside the reference rectangle: the candidates are
     * C1 only (C2/C3 cannot exist geometrically; the rule makes it exact) */
    if (inside == 4) goto select;
    /* C2 */
    real det = FMA(e1u, e2v, -(e1v * e2u));
    real idet = RC(1) / det;
    for (int c = 0; c < 4; ++c) {
        real X = (c == 0 || c == 3) ? hu : -hu;
        real Y = (c < 2) ? hv : -hv;
        real ru = X - cu, rv = Y - cv;
        real al = FMA(ru, e2v, -(rv * e2u)) * idet;
        real be = FMA(e1u, rv, -(e1v * ru)) * idet;
        if (FABS(al) < RC(1) && FABS(be) < RC(1)) {
            real dn = FMA(be, e2n, FMA(al, e1n, cn));
            if (dn <= margin) { cand[nc].u = X; cand[nc].v = Y; cand[nc].n = dn; cand[nc].id = 4 + c; ++nc; }
        }
    }
    /* C3 */
    for (int k = 0; k < 4; ++k) {
        cand_t p = P[k], q = P[(k + 1) & 3];
        for (int s = 0; s < 4; ++s) {
            real lim = (s & 1) ? ((s < 2) ? -hu : -hv) : ((s < 2) ? hu : hv);
            real pc = (s < 2) ? p.u : p.v, qc = (s < 2) ? q.u : q.v;
            real dp = pc - lim, dq = qc - lim;
            if (!((dp < RC(0) && dq > RC(0)) || (dp > RC(0) && dq < RC(0)))) continue;
            real t = dp / (dp - dq);
            cand_t x;
            if (s < 2) {
                x.u = lim;
                x.v = FMA(q.v - p.v, t, p.v);
                if (!(FABS(x.v) <= hv)) continue;
            } else {
                x.v = lim;
                x.u = FMA(q.u - p.u, t, p.u);
                if (!(FABS(x.u) <= hu)) continue;
            }
            x.n = FMA(q.n - p.n, t, p.n);
            x.id = 8 + 4 * k + s;
            if (x.n <= margin) cand[nc++] = x;
        }
    }
select:;
    int sel[24];
    for (int k = 0; k < nc; ++k) sel[k] = 1;
    if (nc > 4) {
        for (int k = 0; k < nc; ++k) sel[k] = 0;
        int i0 = 0;
        for (int k = 1; k < nc; ++k) if (cand[k].n < cand[i0].n) i0 = k;
        int i1 = -1; real bd = RC(0);
        for (int k = 0; k < nc; ++k) {
            if (k == i0) continue;
            real du = cand[k].u - cand[i0].u, dv = cand[k].v - cand[i0].v;
            real d2 = FMA(du, du, dv * dv);
            if (i1 < 0 || d2 > bd) { i1 = k; bd = d2; }
        }
        real ex = cand[i1].u - cand[i0].u, ey = cand[i1].v - cand[i0].v;
        int i2 = -1, i3 = -1; real ba = RC(0), bb = RC(0);
        for (int k = 0; k < nc; ++k) {
            if (k == i0 || k == i1) continue;
            real ar = FMA(ex, cand[k].v - cand[i0].v, -(ey * (cand[k].u - cand[i0].u)));
            if (i2 < 0 || ar > ba) { i2 = k; ba = ar; }
        }
        for (int k = 0; k < nc; ++k) {
            if (k == i0 || k == i1 || k == i2) continue;
            real ar = FMA(ex, cand[k].v - cand[i0].v, -(ey * (cand[k].u - cand[i0].u)));
            if (i3 < 0 || ar < bb) { i3 = k; bb = ar; }
        }
        sel[i0] = sel[i1] = sel[i2] = sel[i3] = 1;
    }
    int m = 0;
    for (int k = 0; k < nc; ++k) {
        if (!sel[k]) continue;
        v3 pw = madd(madd(madd(fc, u, cand[k].u), v, cand[k].v), nr, cand[k].n * RC(0.5));
        pts[m] = pw;
        dist[m] = cand[k].n;
        fid[m] = cand[k].id;
        ++m;
    }
    return m;
}

/* Box-box narrowphase (separating-axis test over 15 axes + face clipping or
 * edge-edge closest points).  Normal n points from A to B.  Returns #points. */
static int box_box(const box_t* A, const box_t* B, real margin, real edge_bias,
                   v3* n_out, v3 pts[4], real dist[4], int ids[4]) {
    v3 d = sub(B->c, A->c);
    real C[3][3], AC[3][3], da[3], db[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { C[i][j] = dot(A->ax[i], B->ax[j]); AC[i][j] = FABS(C[i][j]); }
    for (int i = 0; i < 3; ++i) { da[i] = dot(d, A->ax[i]); db[i] = dot(d, B->ax[i]); }

    real best = RC(0);
    int kind = 0, bi = 0, bj = 0;   /* kind 0: face of A, 1: face of B, 2: edge */
    v3 bax = mk(RC(0), RC(0), RC(0));
    for (int i = 0; i < 3; ++i) {
        real pr = FMA(B->h[0], AC[i][0], FMA(B->h[1], AC[i][1], B->h[2] * AC[i][2]));
        real s = FABS(da[i]) - (A->h[i] + pr);
        if (s > margin) return 0;
        if (i == 0 || s > best) { best = s; kind = 0; bi = i; }
    }
    for (int j = 0; j < 3; ++j) {
        real pr = FMA(A->h[0], AC[0][j], FMA(A->h[1], AC[1][j], A->h[2] * AC[2][j]));
        real s = FABS(db[j]) - (B->h[j] + pr);
        if (s > margin) return 0;
        if (s > best) { best = s; kind = 1; bj = j; }
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            v3 ax = cross(A->ax[i], B->ax[j]);
            real L2 = dot(ax, ax);
            if (L2 < RC(1e-6)) continue;
            real L = SQRT(L2);
            int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            real ra = FMA(A->h[i1], AC[i2][j], A->h[i2] * AC[i1][j]);
            real rb = FMA(B->h[j1], AC[i][j2], B->h[j2] * AC[i][j1]);
            real num = FABS(dot(d, ax)) - (ra + rb);      /* separation * L */
            if (num > margin * L) return 0;
            if (num > (best + edge_bias) * L) { best = num / L; kind = 2; bi = i; bj = j; bax = ax; }
        }
    }
    if (kind == 0) {
        real sg = (da[bi] >= RC(0)) ? RC(1) : RC(-1);
        v3 nr = scl(A->ax[bi], sg);
        *n_out = nr;
        int m = face_contact(A, bi, nr, B, margin, pts, dist, ids);
        for (int k = 0; k < m; ++k) ids[k] += bi * 32;
        return m;
    }
    if (kind == 1) {
        real sg = (db[bj] >= RC(0)) ? RC(-1) : RC(1);
        v3 nr = scl(B->ax[bj], sg);
        *n_out = neg(nr);
        int m = face_contact(B, bj, nr, A, margin, pts, dist, ids);
        for (int k = 0; k < m; ++k) ids[k] += (3 + bj) * 32;
        return m;
    }
    /* edge-edge */
    real L = SQRT(dot(bax, bax));
    v3 w = mk(bax.x / L, bax.y / L, bax.z / L);
    if (dot(w, d) < RC(0)) w = neg(w);
    *n_out = w;
    v3 pa = A->c, pb = B->c;
    for (int k = 0; k < 3; ++k) {
        if (k == bi) continue;
        real sg = (dot(A->ax[k], w) > RC(0)) ? RC(1) : RC(-1);
        pa = madd(pa, A->ax[k], sg * A->h[k]);
    }
    for (int k = 0; k < 3; ++k) {
        if (k == bj) continue;
        real sg = (dot(B->ax[k], w) > RC(0)) ? RC(-1) : RC(1);
        pb = madd(pb, B->ax[k], sg * B->h[k]);
    }
    v3 ua = A->ax[bi], ub = B->ax[bj];
    v3 r = sub(pb, pa);
    real c = dot(ua, ub), ar = dot(ua, r), br = dot(ub, r);
    real den = FMA(-c, c, RC(1));
    real s = FMA(-c, br, ar) / den;
    real t = FMA(c, ar, -br) / den;
    real ha = A->h[bi], hb = B->h[bj];
    s = s > ha ? ha : (s < -ha ? -ha : s);
    t = t > hb ? hb : (t < -hb ? -hb : t);
    v3 qa = madd(pa, ua, s), qb = madd(pb, ub, t);
    pts[0] = scl(add(qa, qb), RC(0.5));
    dist[0] = best;
    ids[0] = 6 * 32 + 3 * bi + bj;
    return 1;
}

static void plane_space(v3 n, v3* t1, v3* t2) {
    if (FABS(n.z) > RC(0.7071067811865476)) {
        real a = FMA(n.y, n.y, n.z * n.z);
        real k = RC(1) / SQRT(a);
        *t1 = mk(RC(0), -(n.z * k), n.y * k);
        *t2 = mk(a * k, -(n.x * t1->z), n.x * t1->y);
    } else {
        real a = FMA(n.x, n.x, n.y * n.y);
        real k = RC(1) / SQRT(a);
        *t1 = mk(-(n.y * k), n.x * k, RC(0));
        *t2 = mk(-(n.z * t1->y), n.z * t1->x, a * k);
    }
}

/* effective inverse mass along direction t for pair (a,b) at lever arm rb */
static real row_k(const sim_t* S, const cp_physics* P, int a, int b, v3 rb, v3 t) {
    int db_ = b - 1;
    real imb = (real)P->inv_mass[b];
    v3 rbt = cross(rb, t);
    v3 ib = symv(S->M[db_], rbt);
    if (a == 0) return imb + dot(rbt, ib);
    int da_ = a - 1;
    real ima = (real)P->inv_mass[a];
    v3 ra = add(rb, sub(S->x[db_], S->x[da_]));
    v3 rat = cross(ra, t);
    v3 ia = symv(S->M[da_], rat);
    return ((ima + imb) + dot(rat, ia)) + dot(rbt, ib);
}

/* One PGS row: Bullet's resolveSingleConstraintRowLowerLimit (normal rows, lambda >= 0)
 * and resolveSingleConstraintRowGeneric (friction rows, |lambda| <= mu * lambda_n) [ext].
 * Returns 1 when the row is NOT converged by Bullet's stopping rule: the row residual is
 * deltaImpulse * (1 / jacDiagABInv) and the solve stops when the max of its square over
 * all rows is <= leastSquaresResidualThreshold (btSequentialImpulseConstraintSolver::
 * solveSingleIteration, pybullet's 1e-7).  With inv_eff = jacDiagABInv > 0 that test is
 * |dl| <= sqrt(threshold) * inv_eff, evaluated here as that product (no division per
 * row; `tol` = sqrt(threshold)).  A friction row whose normal impulse is not > 0 is
 * skipped (Bullet: `if (totalImpulse > 0)`): lambda and the velocities stay as they are
 * and the row adds no residual; written as ln = lam so that it is the kernel's
 * branch-free form. */
static int solve_row(sim_t* S, const cp_physics* P, int a, int b, v3 rb, v3 t,
                     real inv_eff, real target, real* lam, int friction, real bound, real tol) {
    int db_ = b - 1;
    real imb = (real)P->inv_mass[b];
    v3 rbt = cross(rb, t);
    v3 ib = symv(S->M[db_], rbt);
    real vn;
    v3 ia = mk(0, 0, 0), rat = mk(0, 0, 0);
    int da_ = a - 1;
    if (a == 0) {
        vn = dot(t, S->v[db_]) + dot(S->w[db_], rbt);
    } else {
        v3 ra = add(rb, sub(S->x[db_], S->x[da_]));
        rat = cross(ra, t);
        ia = symv(S->M[da_], rat);
        vn = (dot(t, sub(S->v[db_], S->v[da_])) + dot(S->w[db_], rbt)) - dot(S->w[da_], rat);
    }
    real e = target - vn;
    real dl = e * inv_eff;
    real l0 = *lam + dl;
    real ln;
    if (!friction) ln = l0 > RC(0) ? l0 : RC(0);
    else if (bound > RC(0)) ln = l0 > bound ? bound : (l0 < -bound ? -bound : l0);
    else ln = *lam;
    dl = ln - *lam;
    *lam = ln;
    real sb = dl * imb;
    S->v[db_] = madd(S->v[db_], t, sb);
    S->w[db_] = madd(S->w[db_], ib, dl);
    if (a != 0) {
        real sa = dl * (real)P->inv_mass[a];
        S->v[da_] = madd(S->v[da_], neg(t), sa);
        S->w[da_] = madd(S->w[da_], neg(ia), dl);
    }
    return FABS(dl) > tol * inv_eff;
}

/* velocity change of an impulse lam along t at lever arm rb (warm start) */
static void apply_impulse(sim_t* S, const cp_physics* P, int a, int b, v3 rb, v3 t, real lam) {
    int db_ = b - 1;
    v3 rbt = cross(rb, t);
    v3 ib = symv(S->M[db_], rbt);
    S->v[db_] = madd(S->v[db_], t, lam * (real)P->inv_mass[b]);
    S->w[db_] = madd(S->w[db_], ib, lam);
    if (a != 0) {
        int da_ = a - 1;
        v3 ra = add(rb, sub(S->x[db_], S->x[da_]));
        v3 rat = cross(ra, t);
        v3 ia = symv(S->M[da_], rat);
        S->v[da_] = madd(S->v[da_], neg(t), lam * (real)P->inv_mass[a]);
        S->w[da_] = madd(S->w[da_], neg(ia), lam);
    }
}

/* per-island contact storage (one kernel lane's LDS pool) */
typedef struct {
    manifold_t man[CP_ISLAND_PAIRS];
    point_t pt[CP_ISLAND_POINTS];
    fpoint_t fp[CP_ISLAND_FRICTION];
    int used, fused;
} island_t;

#ifdef ORC_STATS
/* one line per island solve: cnt of local pairs 0..4, fcnt of 0..4, merged, sweeps (stdout of a
 * single-threaded run; env order, then substep, then island) */
static FILE* orc_stats_f = NULL;
void orc_stats_open(const char* path) {  /* NULL: stop recording */
    if (orc_stats_f) fclose(orc_stats_f);
    orc_stats_f = path ? fopen(path, "w") : NULL;
}
static void orc_stats_island(const island_t* I, int merged, int it) {
    FILE* f = orc_stats_f;
    if (!f) return;
    for (int j = 0; j < CP_ISLAND_PAIRS; ++j) fprintf(f, "%d ", I->man[j].cnt);
    for (int j = 0; j < CP_ISLAND_PAIRS; ++j) fprintf(f, "%d ", I->man[j].fcnt);
    fprintf(f, "%d %d", merged, it);
    /* per pair: 1 when the manifold normal is exactly +z (the ground's top face is the reference) */
    for (int j = 0; j < CP_ISLAND_PAIRS; ++j)
        fprintf(f, " %d", I->man[j].n.x == RC(0) && I->man[j].n.y == RC(0) && I->man[j].n.z == RC(1));
    fprintf(f, "\n");
}
#endif

/* row sweep helpers: the normal rows, or the friction rows, of local pair j; *bad |= a row
 * above the residual tolerance */
static void sweep_normal(sim_t* S, const cp_physics* P, island_t* I, int isl, int j, real tol, int* bad) {
    int g = ISLAND_PAIR[isl][j];
    int a = PAIR_A[g], b = PAIR_B[g];
    manifold_t* m = &I->man[j];
    for (int k = 0; k < m->cnt; ++k) {
        point_t* q = &I->pt[m->base + k];
        *bad |= solve_row(S, P, a, b, q->rb, q->n, q->inv_eff, q->target, &q->lam, 0, RC(0), tol);
    }
}
static void sweep_friction(sim_t* S, const cp_physics* P, island_t* I, int isl, int j, real tol, int* bad) {
    manifold_t* m = &I->man[j];
    if (m->fcnt == 0) return;
    int g = ISLAND_PAIR[isl][j];
    int a = PAIR_A[g], b = PAIR_B[g];
    for (int k = 0; k < m->fcnt; ++k) {
        point_t* q = &I->pt[m->base + k];
        fpoint_t* f = &I->fp[m->fbase + k];
        real bound = m->mu * q->lam;
        *bad |= solve_row(S, P, a, b, q->rb, f->t1, f->inv_eff1, RC(0), &f->lam1, 1, bound, tol);
        *bad |= solve_row(S, P, a, b, q->rb, f->t2, f->inv_eff2, RC(0), &f->lam2, 1, bound, tol);
    }
}
static void warm_pair(sim_t* S, const cp_physics* P, island_t* I, int isl, int j) {
    int g = ISLAND_PAIR[isl][j];
    int a = PAIR_A[g], b = PAIR_B[g];
    manifold_t* m = &I->man[j];
    for (int k = 0; k < m->cnt; ++k) {
        point_t* q = &I->pt[m->base + k];
        apply_impulse(S, P, a, b, q->rb, q->n, q->lam);
    }
}

#ifdef ORC_DOUBLE
#define ORC_SIMD_EPSILON 2.2204460492503131e-16   /* btScalar double: DBL_EPSILON */
#else
#define ORC_SIMD_EPSILON 1.1920928955078125e-07f  /* btScalar float: FLT_EPSILON */
#endif

/* world point of a box-local point and back (the ground box has identity axes at the origin) */
static inline v3 box_to_world(const box_t* B, v3 l) { return add(B->c, rot(B->ax, l)); }
static inline v3 box_to_local(const box_t* B, v3 w) { return rot_t(B->ax, sub(w, B->c)); }

/* btPersistentManifold::sortCachedPoints (gContactCalcArea3Points, KEEP_DEEPEST_POINT): the
 * cache slot the new point replaces when 4 points are cached -- never the deepest point, else
 * the one whose removal leaves the largest area (in A's local frame); first maximum wins. */
static int pm_sort_cached(const pman_t* M, v3 la, real d) {
    int deepest = -1;
    real maxpen = d;
    for (int i = 0; i < 4; ++i)
        if (M->d[i] < maxpen) { deepest = i; maxpen = M->d[i]; }
    real res[4] = {RC(0), RC(0), RC(0), RC(0)};
    static const int O[4][3] = {{1, 3, 2}, {0, 3, 2}, {0, 3, 1}, {0, 2, 1}};  /* a = new - [0]; b = [1] - [2] */
    for (int i = 0; i < 4; ++i) {
        if (i == deepest) continue;
        v3 a0 = sub(la, M->la[O[i][0]]);
        v3 b0 = sub(M->la[O[i][1]], M->la[O[i][2]]);
        v3 c = cross(a0, b0);
        res[i] = dot(c, c);
    }
    int best = -1;
    real bv = -RC(1e30);
    for (int i = 0; i < 4; ++i)
        if (FABS(res[i]) > bv) { bv = FABS(res[i]); best = i; }
    return best;
}

/* CP_MODEL_PERSISTENT: Bullet's box-box collision of one pair with a persistent manifold
 * (btBoxBoxCollisionAlgorithm::processCollision with USE_PERSISTENT_CONTACTS):
 *   1. new points from the box-box detector, which reports overlapping boxes only (dBoxBox2
 *      returns nothing for a separating axis; penetrating candidates only): box_box at margin 0;
 *   2. each new point (btManifoldResult::addContactPoint): getCacheEntry -- the cached point
 *      nearest in A's local frame within the breaking threshold -- is replaced, keeping its
 *      applied impulse (replaceContactPoint, MAINTAIN_PERSISTENCY); else the point is added, a
 *      5th one replacing the slot sortCachedPoints picks;
 *   3. refreshContactPoints: every cached point's world positions from its local points and the
 *      current poses, its separation along its own normal; points separated by more than the
 *      breaking threshold, or drifted sideways by more than it, are removed (last slot moved in).
 * The breaking threshold is relative (btCollisionDispatcher's default
 * CD_USE_RELATIVE_CONTACT_BREAKING_THRESHOLD): gContactBreakingThreshold (contact_margin, 0.02)
 * times the smaller of the two shapes' getAngularMotionDisc (the bounding-sphere radius |h| of a
 * box centred in its link frame): 2.9 mm for the cart pairs, 5.0 mm for pole-ground and
 * pole-pole, 2.9 mm for cart-pole.  Returns the
 * cached points as rows: the point on B (the solver's lever point for both bodies here; Bullet
 * uses A's own point for A, which moves only the friction rows' lever arms, by d along n), its
 * normal (A -> B) and separation. */
static int persistent_manifold(pman_t* M, const box_t* A, const box_t* B, const cp_physics* P, v3 pts[4],
                               v3 nrm[4], real dist[4]) {
    const real ra = SQRT(dot(mk(A->h[0], A->h[1], A->h[2]), mk(A->h[0], A->h[1], A->h[2])));
    const real rb = SQRT(dot(mk(B->h[0], B->h[1], B->h[2]), mk(B->h[0], B->h[1], B->h[2])));
    const real thr = (real)P->contact_margin * (ra < rb ? ra : rb);
    v3 n, np[4];
    real nd[4];
    int nid[4];
    int cnt = box_box(A, B, RC(0), (real)P->edge_bias, &n, np, nd, nid);
    for (int k = 0; k < cnt; ++k) {
        v3 pa = madd(np[k], n, -(nd[k] * RC(0.5)));   /* on A's surface */
        v3 pb = madd(np[k], n, nd[k] * RC(0.5));      /* on B's surface */
        v3 la = box_to_local(A, pa), lb = box_to_local(B, pb);
        real best = thr * thr;
        int idx = -1;
        for (int c = 0; c < M->cnt; ++c) {
            v3 df = sub(M->la[c], la);
            real d2 = dot(df, df);
            if (d2 < best) { best = d2; idx = c; }
        }
        real lam = RC(0);
        if (idx >= 0) {
            lam = M->lam[idx];
        } else if (M->cnt == 4) {
            idx = pm_sort_cached(M, la, nd[k]);
        } else {
            idx = M->cnt++;
        }
        M->la[idx] = la;
        M->lb[idx] = lb;
        M->n[idx] = n;
        M->d[idx] = nd[k];
        M->lam[idx] = lam;
    }
    for (int c = M->cnt - 1; c >= 0; --c) {
        v3 pa = box_to_world(A, M->la[c]), pb = box_to_world(B, M->lb[c]);
        real d = dot(sub(pb, pa), M->n[c]);
        int keep = d <= thr;
        if (keep) {
            v3 proj = madd(pa, M->n[c], d);
            v3 df = sub(pb, proj);
            keep = dot(df, df) <= thr * thr;
        }
        if (keep) {
            M->d[c] = d;
        } else {
            int last = M->cnt - 1;
            if (c != last) {
                M->la[c] = M->la[last]; M->lb[c] = M->lb[last]; M->n[c] = M->n[last];
                M->d[c] = M->d[last]; M->lam[c] = M->lam[last];
            }
            M->cnt--;
        }
    }
    for (int c = 0; c < M->cnt; ++c) {
        pts[c] = box_to_world(B, M->lb[c]);
        nrm[c] = M->n[c];
        dist[c] = M->d[c];
    }
    return M->cnt;
}

/* btMultiBody::applyDeltaVeeMultiDof [ext]: every base velocity coordinate (world angular
 * x, y, z, then linear x, y, z) is clamped to +-m_maxCoordinateVelocity whenever a velocity
 * change is applied to it (btClamp: `if (a < lb) a = lb; else if (ub < a) a = ub;`, so a NaN
 * passes through).  Bounds the loose pole's yaw spin, whose explicit gyroscopic term otherwise
 * diverges. */
static inline real clamp_coord(real a, real lim) { return a < -lim ? -lim : (lim < a ? lim : a); }
static void clamp_velocities(sim_t* S, const cp_physics* P) {
    const real lim = (real)P->max_coord_velocity;
    if (!(lim > RC(0))) return;
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        S->w[d] = mk(clamp_coord(S->w[d].x, lim), clamp_coord(S->w[d].y, lim), clamp_coord(S->w[d].z, lim));
        S->v[d] = mk(clamp_coord(S->v[d].x, lim), clamp_coord(S->v[d].y, lim), clamp_coord(S->v[d].z, lim));
    }
}

/* ---- CP_MODEL_SLEEPING: Bullet's deactivation, restated [ext].
 * Islands: btSimulationIslandManager::findUnions unites the non-static bodies of every broadphase
 * pair, i.e. every pair whose AABBs overlap; an AABB is btTransformAabb of the box (world extent
 * along axis k = sum_c |R_kc| h_c) grown by gContactBreakingThreshold (btCollisionWorld::
 * updateSingleAabb; here contact_margin, 0.02 m).  The static ground joins nothing. */
static void body_aabb(const sim_t* S, const cp_physics* P, int d, v3* lo, v3* hi) {
    const float* h = P->half_extents[d + 1];
    const v3* ax = S->ax[d];   /* ax[c] = world coordinates of local axis c: R_kc = ax[c].k */
    const real thr = (real)P->contact_margin;
    const real ex = ((real)h[0] * FABS(ax[0].x) + (real)h[1] * FABS(ax[1].x)) + (real)h[2] * FABS(ax[2].x);
    const real ey = ((real)h[0] * FABS(ax[0].y) + (real)h[1] * FABS(ax[1].y)) + (real)h[2] * FABS(ax[2].y);
    const real ez = ((real)h[0] * FABS(ax[0].z) + (real)h[1] * FABS(ax[1].z)) + (real)h[2] * FABS(ax[2].z);
    const v3 c = S->x[d];
    *lo = mk((c.x - ex) - thr, (c.y - ey) - thr, (c.z - ez) - thr);
    *hi = mk((c.x + ex) + thr, (c.y + ey) + thr, (c.z + ez) + thr);
}
/* btSimulationIslandManager::buildIslands' activation pass: an island none of whose bodies is
 * ACTIVE_TAG goes to ISLAND_SLEEPING as a whole; in an island with an ACTIVE_TAG body, the sleeping
 * ones become WANTS_DEACTIVATION (simulated again).  Run at the start of the step, from the poses
 * and the states left by the previous step's updateActivationState (the narrowphase does not
 * change either). */
static void sleep_islands(sim_t* S, const cp_physics* P) {
    v3 lo[CP_NUM_DYN], hi[CP_NUM_DYN];
    for (int d = 0; d < CP_NUM_DYN; ++d) body_aabb(S, P, d, &lo[d], &hi[d]);
    int root[CP_NUM_DYN] = {0, 1, 2, 3};
    for (int a = 0; a < CP_NUM_DYN; ++a)
        for (int b = a + 1; b < CP_NUM_DYN; ++b) {
            const int ov = !(lo[a].x > hi[b].x || hi[a].x < lo[b].x || lo[a].y > hi[b].y || hi[a].y < lo[b].y ||
                             lo[a].z > hi[b].z || hi[a].z < lo[b].z);   /* btAabbOverlap */
            if (!ov) continue;
            const int ra = root[a], rb = root[b];
            if (ra == rb) continue;
            const int lo_r = ra < rb ? ra : rb, hi_r = ra < rb ? rb : ra;
            for (int d = 0; d < CP_NUM_DYN; ++d) if (root[d] == hi_r) root[d] = lo_r;
        }
    for (int r = 0; r < CP_NUM_DYN; ++r) {
        int any_active = 0;
        for (int d = 0; d < CP_NUM_DYN; ++d)
            if (root[d] == r && (S->slp_a[d] & 15) == CP_ACT_ACTIVE) any_active = 1;
        for (int d = 0; d < CP_NUM_DYN; ++d) {
            if (root[d] != r) continue;
            const int32_t aw = S->slp_a[d] & CP_ACT_AWAKE;
            if (!any_active) S->slp_a[d] = CP_ACT_SLEEPING | aw;
            else if ((S->slp_a[d] & 15) == CP_ACT_SLEEPING) S->slp_a[d] = CP_ACT_WANTS | aw;
        }
    }
}
/* the end of the step: btMultiBody::checkMotionAndSleepIfRequired (motion = the squared base
 * velocity coordinates, angular then linear, summed in order; below SLEEP_EPSILON the sleep timer
 * runs and past SLEEP_TIMEOUT the body stops being awake, else the timer restarts and the body is
 * awake), then btMultiBodyDynamicsWorld::updateActivationState (not awake and ACTIVE_TAG ->
 * WANTS_DEACTIVATION; awake -> ACTIVE_TAG) */
static void sleep_update(sim_t* S, const cp_physics* P) {
    const real dt = (real)P->dt, eps = (real)P->sleep_epsilon, tmo = (real)P->sleep_timeout;
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        const v3 w = S->w[d], v = S->v[d];
        const real motion = ((((w.x * w.x + w.y * w.y) + w.z * w.z) + v.x * v.x) + v.y * v.y) + v.z * v.z;
        int32_t a = S->slp_a[d];
        if (motion < eps) {
            S->slp_t[d] = S->slp_t[d] + dt;
            if (S->slp_t[d] > tmo) a &= ~CP_ACT_AWAKE;
        } else {
            S->slp_t[d] = RC(0);
            a |= CP_ACT_AWAKE;
        }
        if (a & CP_ACT_AWAKE) a = CP_ACT_ACTIVE | CP_ACT_AWAKE;
        else if ((a & 15) == CP_ACT_ACTIVE) a = CP_ACT_WANTS;
        S->slp_a[d] = a;
    }
}
static void sleep_wake_all(sim_t* S) {   /* resetBasePositionAndOrientation [ext, low confidence] */
    for (int d = 0; d < CP_NUM_DYN; ++d) { S->slp_a[d] = CP_ACT_ACTIVE | CP_ACT_AWAKE; S->slp_t[d] = RC(0); }
}

/* one p.stepSimulation() of the scene (DESIGN.md §Physics model, steps 1-8) */
static void substep(sim_t* S, const cp_physics* P, int32_t* overflow, int32_t* iters_out, int32_t* npts_out,
                    int32_t* isl_iters, int32_t* merged_out) {
    const real dt = (real)P->dt, inv_dt = (real)P->inv_dt;
    /* 1. orientation matrices, world inverse inertia */
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        quat_axes(S->q[d], S->ax[d]);
        world_inv_inertia(S->ax[d], P->inv_inertia[d + 1], S->M[d]);
    }
    /* 1b. CP_MODEL_SLEEPING: this step's island activation; a sleeping body is not simulated */
    const int sleeping = (P->model_flags & CP_MODEL_SLEEPING) != 0;
    int sl[CP_NUM_DYN] = {0, 0, 0, 0};
    if (sleeping) {
        sleep_islands(S, P);
        for (int d = 0; d < CP_NUM_DYN; ++d) sl[d] = (S->slp_a[d] & 15) == CP_ACT_SLEEPING;
    }
    int skip[CP_NUM_ISLANDS][CP_ISLAND_PAIRS];   /* pairs of a sleeping island: no contact, cache kept */
    /* 2. narrowphase + row setup at the start-of-step poses, per island: its 3 own
     *    pairs then its 2 cross pairs, into its own capped pool */
    const int persistent = (P->model_flags & CP_MODEL_PERSISTENT) != 0;
    island_t isl[CP_NUM_ISLANDS];
    for (int p = 0; p < CP_NUM_ISLANDS; ++p) {
        island_t* I = &isl[p];
        I->used = I->fused = 0;
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            int g = ISLAND_PAIR[p][j];
            int a = PAIR_A[g], b = PAIR_B[g];
            box_t A, B;
            get_box(S, P, a, &A);
            get_box(S, P, b, &B);
            v3 n, pts[4], pn[4] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            real dist[4];
            int ids[4], pmi[4];
            int cnt;
            skip[p][j] = sl[b - 1] || (a > 0 && sl[a - 1]);
            if (skip[p][j]) {
                cnt = 0;
                n = mk(RC(0), RC(0), RC(1));
            } else if (!persistent) {
                cnt = box_box(&A, &B, (real)P->contact_margin, (real)P->edge_bias, &n, pts, dist, ids);
                for (int k = 0; k < cnt; ++k) { pn[k] = n; pmi[k] = -1; }
            } else {
                cnt = persistent_manifold(&S->pm[p][j], &A, &B, P, pts, pn, dist);
                n = cnt ? pn[0] : mk(RC(0), RC(0), RC(1));
                for (int k = 0; k < cnt; ++k) { ids[k] = k; pmi[k] = k; }
            }
            int m = cnt < CP_ISLAND_POINTS - I->used ? cnt : CP_ISLAND_POINTS - I->used;
            *overflow += cnt - m;
            manifold_t* man = &I->man[j];
            man->n = n;
            man->cnt = m;
            man->base = I->used;
            man->mu = (real)P->friction[a] * (real)P->friction[b];
            man->fcnt = 0;
            man->fbase = I->fused;
            for (int k = 0; k < m; ++k) {
                point_t* q = &I->pt[I->used + k];
                q->rb = sub(pts[k], S->x[b - 1]);
                q->n = pn[k];
                real K = row_k(S, P, a, b, q->rb, pn[k]);
                q->inv_eff = RC(1) / K;
                q->target = dist[k] > RC(0) ? -(dist[k] * inv_dt) : -(((real)P->erp * dist[k]) * inv_dt);
                q->id = ids[k];
                q->pm = pmi[k];
                real l0 = RC(0);
                if (!persistent) {  /* warm start: impulse of the same feature in the last substep */
                    for (int q4 = 0; q4 < 4; ++q4) {
                        if ((int)((S->ws_id[p][j] >> (8 * q4)) & 0xFFu) == ids[k]) { l0 = S->ws_lam[p][j][q4]; break; }
                    }
                } else {            /* the cached point's applied impulse */
                    l0 = S->pm[p][j].lam[k];
                }
                q->lam = (real)P->warmstart * l0;
            }
            if (man->mu > RC(0) && m > 0) {  /* friction rows: directions and masses after step 3 */
                int fm = m < CP_ISLAND_FRICTION - I->fused ? m : CP_ISLAND_FRICTION - I->fused;
                *overflow += m - fm;
                man->fcnt = fm;
                I->fused += fm;
            }
            I->used += m;
        }
    }
    /* 3. unconstrained velocity update: gravity + pending force + Bullet multibody
     *    damping (-m v (k + k|v|), -I w (k + k|w|)) + gyroscopic term */
    const real kl = (real)P->lin_damping, ka = (real)P->ang_damping;
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        if (sl[d]) continue;   /* CP_MODEL_SLEEPING: no gravity, forces or damping for a sleeping body */
        int g = d + 1;
        real im = (real)P->inv_mass[g];
        v3 v = S->v[d], w = S->w[d], F = S->f[d];
        real vlen = SQRT(dot(v, v));
        real dv = FMA(kl, vlen, kl);
        v3 acc = mk(FMA(-v.x, dv, FMA(F.x, im, (real)P->gravity[0])),
                    FMA(-v.y, dv, FMA(F.y, im, (real)P->gravity[1])),
                    FMA(-v.z, dv, FMA(F.z, im, (real)P->gravity[2])));
        v3 wl = rot_t(S->ax[d], w);
        v3 Iwl = mk((real)P->inertia[g][0] * wl.x, (real)P->inertia[g][1] * wl.y, (real)P->inertia[g][2] * wl.z);
        v3 gl = cross(wl, Iwl);
        v3 al = mk(-((real)P->inv_inertia[g][0] * gl.x), -((real)P->inv_inertia[g][1] * gl.y),
                   -((real)P->inv_inertia[g][2] * gl.z));
        v3 aw = rot(S->ax[d], al);
        real wlen = SQRT(dot(w, w));
        real dw = FMA(ka, wlen, ka);
        v3 accw = mk(FMA(-w.x, dw, aw.x), FMA(-w.y, dw, aw.y), FMA(-w.z, dw, aw.z));
        S->v[d] = madd(v, acc, dt);
        S->w[d] = madd(w, accw, dt);
    }
    clamp_velocities(S, P);  /* the unconstrained update goes through applyDeltaVeeMultiDof(output, dt) */
    /* 3b. friction rows (the rows' masses depend on positions only, so setting them up after
     *     the velocity update changes no value of the default model).  Directions: btPlaneSpace1
     *     of the normal; CP_MODEL_VEL_FRICTION: the lateral relative velocity at the point when
     *     its length^2 exceeds SIMD_EPSILON, the second direction its cross with Bullet's normal
     *     (convertContact of the rigid-body solver), else btPlaneSpace1. */
    for (int p = 0; p < CP_NUM_ISLANDS; ++p) {
        island_t* I = &isl[p];
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            manifold_t* man = &I->man[j];
            int g = ISLAND_PAIR[p][j];
            int a = PAIR_A[g], b = PAIR_B[g];
            for (int k = 0; k < man->fcnt; ++k) {
                point_t* q = &I->pt[man->base + k];
                fpoint_t* f = &I->fp[man->fbase + k];
                v3 t1, t2;
                plane_space(q->n, &t1, &t2);
                if (P->model_flags & CP_MODEL_VEL_FRICTION) {
                    v3 vb = add(S->v[b - 1], cross(S->w[b - 1], q->rb));
                    v3 va = mk(RC(0), RC(0), RC(0));
                    if (a != 0) {
                        v3 ra = add(q->rb, sub(S->x[b - 1], S->x[a - 1]));
                        va = add(S->v[a - 1], cross(S->w[a - 1], ra));
                    }
                    v3 vel = sub(va, vb);
                    v3 lat = madd(vel, q->n, -dot(q->n, vel));
                    real l2 = dot(lat, lat);
                    if (l2 > ORC_SIMD_EPSILON) {
                        real il = RC(1) / SQRT(l2);
                        t1 = scl(lat, il);
                        v3 c = cross(t1, neg(q->n));
                        real cl = RC(1) / SQRT(dot(c, c));
                        t2 = scl(c, cl);
                    }
                }
                f->t1 = t1;
                f->t2 = t2;
                f->inv_eff1 = RC(1) / row_k(S, P, a, b, q->rb, t1);
                f->inv_eff2 = RC(1) / row_k(S, P, a, b, q->rb, t2);
                f->lam1 = f->lam2 = RC(0);
            }
        }
    }
    /* 4. warm start + projected Gauss-Seidel over ONE solver group per env.  Bullet's
     *    island manager batches islands into one solve until the group holds
     *    m_minimumSolverBatchSize (128) constraints [ext], so the two cart-pole islands
     *    (<= 40 rows together) are one solve with one stopping decision: the sweep runs
     *    every normal row, then every friction row, and stops after the sweep whose
     *    largest squared row residual is <= leastSquaresResidualThreshold
     *    (solve_row), or after solver_iterations sweeps.  Without a cross-island contact
     *    the rows of the two islands touch disjoint bodies, so island 0's sweep then
     *    island 1's gives the same numbers as their rows interleaved; with one, the
     *    order is 0 2 1 3 4 9 5 6 7 8 (normal rows, then friction rows). */
    const int iters = P->solver_iterations;
    const real tol = SQRT((real)P->residual_threshold);
    int merged = 0;
    for (int p = 0; p < CP_NUM_ISLANDS; ++p) merged |= (isl[p].man[3].cnt + isl[p].man[4].cnt) > 0;
    if (merged_out) *merged_out += merged;
    int it = 0;
    if (!merged && (P->model_flags & CP_MODEL_SPLIT_ISLANDS)) {
        /* one solver group per island (m_minimumSolverBatchSize <= 1): own warm start, own
         * stopping decision; the islands share no dynamic body, so their order is immaterial */
        for (int p = 0; p < CP_NUM_ISLANDS; ++p) {
            for (int j = 0; j < 3; ++j) warm_pair(S, P, &isl[p], p, j);
            if (isl[p].used == 0) continue;
            int itp;
            for (itp = 0; itp < iters;) {
                int bad = 0;
                for (int j = 0; j < 3; ++j) sweep_normal(S, P, &isl[p], p, j, tol, &bad);
                for (int j = 0; j < 3; ++j) sweep_friction(S, P, &isl[p], p, j, tol, &bad);
                ++itp;
                if (!bad) break;
            }
            if (itp > it) it = itp;
        }
    } else if (!merged) {
        for (int p = 0; p < CP_NUM_ISLANDS; ++p)
            for (int j = 0; j < 3; ++j) warm_pair(S, P, &isl[p], p, j);
        if (isl[0].used + isl[1].used > 0) {
            for (it = 0; it < iters;) {
                int bad = 0;
                for (int p = 0; p < CP_NUM_ISLANDS; ++p) {
                    for (int j = 0; j < 3; ++j) sweep_normal(S, P, &isl[p], p, j, tol, &bad);
                    for (int j = 0; j < 3; ++j) sweep_friction(S, P, &isl[p], p, j, tol, &bad);
                }
                ++it;
#ifdef ORC_DEBUG
                if (getenv("ORC_DEBUG")) fprintf(stderr, "it %d bad %d\n", it, bad);
#endif
                if (!bad) break;
            }
        }
    } else {
        /* global order: (0,0) (1,0) (0,1) (1,1) (0,2) (1,2) then cross (0,3) (0,4) (1,3) (1,4) */
        static const int ORD_I[10] = {0, 1, 0, 1, 0, 1, 0, 0, 1, 1};
        static const int ORD_J[10] = {0, 0, 1, 1, 2, 2, 3, 4, 3, 4};
        for (int o = 0; o < 10; ++o) warm_pair(S, P, &isl[ORD_I[o]], ORD_I[o], ORD_J[o]);
        for (it = 0; it < iters;) {
            int bad = 0;
            for (int o = 0; o < 10; ++o) sweep_normal(S, P, &isl[ORD_I[o]], ORD_I[o], ORD_J[o], tol, &bad);
            for (int o = 0; o < 10; ++o) sweep_friction(S, P, &isl[ORD_I[o]], ORD_I[o], ORD_J[o], tol, &bad);
            ++it;
            if (!bad) break;
        }
    }
    const int it_max = it;
    if (isl_iters)
        for (int p = 0; p < CP_NUM_ISLANDS; ++p)
            if (it > isl_iters[p]) isl_iters[p] = it;
#ifdef ORC_STATS  /* diagnostic build only (tools/row_classes.py): row structure + sweeps per island */
    for (int p = 0; p < CP_NUM_ISLANDS; ++p) orc_stats_island(&isl[p], merged, it);
#endif
    /* 4c. refresh the warm-start cache (CP_MODEL_PERSISTENT: the cached points' impulses) */
    for (int p = 0; p < CP_NUM_ISLANDS; ++p)
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            const manifold_t* m = &isl[p].man[j];
            for (int k = 0; k < m->cnt; ++k) {
                const point_t* q = &isl[p].pt[m->base + k];
                if (q->pm >= 0) S->pm[p][j].lam[q->pm] = q->lam;
            }
        }
    for (int p = 0; p < CP_NUM_ISLANDS && !persistent; ++p) {   /* feature-id cache: default model only */
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            if (skip[p][j]) continue;   /* a sleeping island's manifolds keep their impulses */
            manifold_t* m = &isl[p].man[j];
            uint32_t idw = 0xFFFFFFFFu;
            for (int k = 0; k < 4; ++k) {
                if (k < m->cnt) {
                    point_t* q = &isl[p].pt[m->base + k];
                    idw = (idw & ~(0xFFu << (8 * k))) | ((uint32_t)q->id << (8 * k));
                    S->ws_lam[p][j][k] = q->lam;
                } else {
                    S->ws_lam[p][j][k] = RC(0);
                }
            }
            S->ws_id[p][j] = idw;
        }
    }
    /* 4d. the solver's velocity change is written back through applyDeltaVeeMultiDof too */
    clamp_velocities(S, P);
    /* 5. integrate positions (semi-implicit) and orientation (exponential map) */
    const real hdt = RC(0.5) * dt;
    const real c3 = ((dt * dt) * dt) * RC(0.020833333333);
    const real maxang = (real)P->max_angular_step;
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        if (sl[d]) {   /* btMultiBodyDynamicsWorld::integrateTransforms: a sleeping body's velocities cleared */
            S->v[d] = S->w[d] = mk(RC(0), RC(0), RC(0));
            continue;
        }
        v3 v = S->v[d], w = S->w[d];
        S->x[d] = madd(S->x[d], v, dt);
        real ang = SQRT(dot(w, w));
        if (ang * dt > maxang) ang = maxang * inv_dt;
        real half = hdt * ang;
        real sn, cs, s;
        sincos_small(half, &sn, &cs);
        if (ang < RC(0.001)) s = FMA(-c3, ang * ang, hdt);
        else s = sn / ang;
        real dx = w.x * s, dy = w.y * s, dz = w.z * s, dw = cs;
        real* q = S->q[d];
        real qx = q[0], qy = q[1], qz = q[2], qw = q[3];
        real rw = FMA(dw, qw, -FMA(dx, qx, FMA(dy, qy, dz * qz)));
        real rx = FMA(dw, qx, FMA(dx, qw, FMA(dy, qz, -(dz * qy))));
        real ry = FMA(dw, qy, FMA(dy, qw, FMA(dz, qx, -(dx * qz))));
        real rz = FMA(dw, qz, FMA(dz, qw, FMA(dx, qy, -(dy * qx))));
        real n2 = FMA(rx, rx, FMA(ry, ry, FMA(rz, rz, rw * rw)));
        real inv = RC(1) / SQRT(n2);
        q[0] = rx * inv; q[1] = ry * inv; q[2] = rz * inv; q[3] = rw * inv;
    }
    /* 6. external forces are consumed by the step (pybullet clears them) */
    for (int d = 0; d < CP_NUM_DYN; ++d) S->f[d] = mk(RC(0), RC(0), RC(0));
    /* 7. CP_MODEL_SLEEPING: updateActivationState */
    if (sleeping) sleep_update(S, P);
    if (iters_out) *iters_out = it_max;
    if (npts_out) *npts_out = isl[0].used + isl[1].used;
}

/* LINK_FRAME force at the link origin (= COM): world force = R(q) f, no torque
 * (bullet_cartpole.py:202-207, :349-351).  Accumulates until the next step. */
static void apply_force_link(sim_t* S, int d, real fx, real fy, real fz) {
    v3 ax[3];
    quat_axes(S->q[d], ax);
    S->f[d] = add(S->f[d], rot(ax, mk(fx, fy, fz)));
}

/* ------------------------------------------------------------ world-level API */
static void world_load(const orc_world* w, sim_t* S) {
    memset(S->pm, 0, sizeof(S->pm));  /* CP_MODEL_PERSISTENT is an env-level (orc_envs) option */
    sleep_wake_all(S);                /* so is CP_MODEL_SLEEPING (its state lives in the env SoA) */
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        S->x[d] = mk((real)w->pos[d][0], (real)w->pos[d][1], (real)w->pos[d][2]);
        for (int k = 0; k < 4; ++k) S->q[d][k] = (real)w->quat[d][k];
        S->v[d] = mk((real)w->vel[d][0], (real)w->vel[d][1], (real)w->vel[d][2]);
        S->w[d] = mk((real)w->omega[d][0], (real)w->omega[d][1], (real)w->omega[d][2]);
        S->f[d] = mk((real)w->pending[d][0], (real)w->pending[d][1], (real)w->pending[d][2]);
    }
    for (int p = 0; p < CP_NUM_ISLANDS; ++p)
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            S->ws_id[p][j] = w->ws_id[p * CP_ISLAND_PAIRS + j];
            for (int k = 0; k < 4; ++k) S->ws_lam[p][j][k] = (real)w->ws_lam[p * CP_ISLAND_PAIRS + j][k];
        }
}
static void world_store(orc_world* w, const sim_t* S) {
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        w->pos[d][0] = S->x[d].x; w->pos[d][1] = S->x[d].y; w->pos[d][2] = S->x[d].z;
        for (int k = 0; k < 4; ++k) w->quat[d][k] = S->q[d][k];
        w->vel[d][0] = S->v[d].x; w->vel[d][1] = S->v[d].y; w->vel[d][2] = S->v[d].z;
        w->omega[d][0] = S->w[d].x; w->omega[d][1] = S->w[d].y; w->omega[d][2] = S->w[d].z;
        w->pending[d][0] = S->f[d].x; w->pending[d][1] = S->f[d].y; w->pending[d][2] = S->f[d].z;
    }
    for (int p = 0; p < CP_NUM_ISLANDS; ++p)
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            w->ws_id[p * CP_ISLAND_PAIRS + j] = S->ws_id[p][j];
            for (int k = 0; k < 4; ++k) w->ws_lam[p * CP_ISLAND_PAIRS + j][k] = S->ws_lam[p][j][k];
        }
}

void orc_world_spawn(orc_world* w, const cp_config* cfg) {
    memset(w, 0, sizeof(*w));
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        for (int k = 0; k < 3; ++k) w->pos[d][k] = cfg->phys.spawn_pos[d + 1][k];
        w->quat[d][3] = 1.0;
    }
    for (int p = 0; p < CP_NUM_PAIRS; ++p) w->ws_id[p] = 0xFFFFFFFFu;
}
void orc_world_reset_pose(orc_world* w, int body, const double p[3], const double q[4]) {
    int d = body - 1;
    if (d < 0 || d >= CP_NUM_DYN) return;
    for (int k = 0; k < 3; ++k) { w->pos[d][k] = (float)p[k]; w->vel[d][k] = 0; w->omega[d][k] = 0; }
    for (int k = 0; k < 4; ++k) w->quat[d][k] = (float)q[k];
}
void orc_world_step(orc_world* w, const cp_config* cfg) {
    sim_t S;
    world_load(w, &S);
    substep(&S, &cfg->phys, &w->overflow, &w->last_iterations, &w->last_points, NULL, NULL);
    world_store(w, &S);
}
void orc_world_apply_force_link(orc_world* w, int body, double fx, double fy, double fz) {
    int d = body - 1;
    if (d < 0 || d >= CP_NUM_DYN) return;
    sim_t S;
    world_load(w, &S);
    apply_force_link(&S, d, (real)(float)fx, (real)(float)fy, (real)(float)fz);
    world_store(w, &S);
}
void orc_world_get_pose(const orc_world* w, int body, double out7[7]) {
    int d = body - 1;
    for (int k = 0; k < 3; ++k) out7[k] = w->pos[d][k];
    for (int k = 0; k < 4; ++k) out7[3 + k] = w->quat[d][k];
}
void orc_world_get_velocity(const orc_world* w, int body, double out6[6]) {
    int d = body - 1;
    for (int k = 0; k < 3; ++k) { out6[k] = w->vel[d][k]; out6[3 + k] = w->omega[d][k]; }
}
void orc_world_get_euler(const orc_world* w, int body, double out3[3]) {
    int d = body - 1;
    real q[4], rpy[3];
    for (int k = 0; k < 4; ++k) q[k] = (real)w->quat[d][k];
    quat_euler(q, rpy);
    for (int k = 0; k < 3; ++k) out3[k] = rpy[k];
}

/* -------------------------------------------------------------- env-level API */
#define SF(e, f, i) (((real*)(e)->state)[(size_t)(f) * (e)->B + (i)])

static void env_load(const orc_envs* e, int i, sim_t* S) {
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        S->x[d] = mk(SF(e, CP_SF_BODY(d, 0), i), SF(e, CP_SF_BODY(d, 1), i), SF(e, CP_SF_BODY(d, 2), i));
        for (int k = 0; k < 4; ++k) S->q[d][k] = SF(e, CP_SF_BODY(d, 3 + k), i);
        S->v[d] = mk(SF(e, CP_SF_BODY(d, 7), i), SF(e, CP_SF_BODY(d, 8), i), SF(e, CP_SF_BODY(d, 9), i));
        S->w[d] = mk(SF(e, CP_SF_BODY(d, 10), i), SF(e, CP_SF_BODY(d, 11), i), SF(e, CP_SF_BODY(d, 12), i));
        S->f[d] = mk(RC(0), RC(0), RC(0));
    }
    for (int c = 0; c < 2; ++c)
        S->f[2 * c] = mk(SF(e, CP_SF_PENDING(c, 0), i), SF(e, CP_SF_PENDING(c, 1), i), SF(e, CP_SF_PENDING(c, 2), i));
    for (int p = 0; p < CP_NUM_ISLANDS; ++p)
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            memcpy(&S->ws_id[p][j], &SF(e, CP_SF_WS_ID(p, j), i), 4);
            for (int k = 0; k < 4; ++k) S->ws_lam[p][j][k] = SF(e, CP_SF_WS_LAM(p, j, k), i);
        }
    memcpy(S->pm, (const pman_t*)e->pman + (size_t)i * CP_NUM_PAIRS, sizeof(S->pm));
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        memcpy(&S->slp_a[d], &SF(e, CP_SF_SLEEP_ACT(d), i), 4);
        S->slp_t[d] = SF(e, CP_SF_SLEEP_TIMER(d), i);
    }
}
static void env_store(orc_envs* e, int i, const sim_t* S) {
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        SF(e, CP_SF_BODY(d, 0), i) = S->x[d].x;
        SF(e, CP_SF_BODY(d, 1), i) = S->x[d].y;
        SF(e, CP_SF_BODY(d, 2), i) = S->x[d].z;
        for (int k = 0; k < 4; ++k) SF(e, CP_SF_BODY(d, 3 + k), i) = S->q[d][k];
        SF(e, CP_SF_BODY(d, 7), i) = S->v[d].x;
        SF(e, CP_SF_BODY(d, 8), i) = S->v[d].y;
        SF(e, CP_SF_BODY(d, 9), i) = S->v[d].z;
        SF(e, CP_SF_BODY(d, 10), i) = S->w[d].x;
        SF(e, CP_SF_BODY(d, 11), i) = S->w[d].y;
        SF(e, CP_SF_BODY(d, 12), i) = S->w[d].z;
    }
    for (int c = 0; c < 2; ++c) {
        SF(e, CP_SF_PENDING(c, 0), i) = S->f[2 * c].x;
        SF(e, CP_SF_PENDING(c, 1), i) = S->f[2 * c].y;
        SF(e, CP_SF_PENDING(c, 2), i) = S->f[2 * c].z;
    }
    for (int p = 0; p < CP_NUM_ISLANDS; ++p)
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            memcpy(&SF(e, CP_SF_WS_ID(p, j), i), &S->ws_id[p][j], 4);
            for (int k = 0; k < 4; ++k) SF(e, CP_SF_WS_LAM(p, j, k), i) = S->ws_lam[p][j][k];
        }
    memcpy((pman_t*)e->pman + (size_t)i * CP_NUM_PAIRS, S->pm, sizeof(S->pm));
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        memcpy(&SF(e, CP_SF_SLEEP_ACT(d), i), &S->slp_a[d], 4);
        SF(e, CP_SF_SLEEP_TIMER(d), i) = S->slp_t[d];
    }
}
static int32_t get_i(const orc_envs* e, int f, int i) {
    int32_t v;
    memcpy(&v, &SF(e, f, i), 4);
    return v;
}
static void set_i(orc_envs* e, int f, int i, int32_t v) { memcpy(&SF(e, f, i), &v, 4); }

static void write_obs_row(const sim_t* S, float* dst /* 14 floats */) {
    for (int o = 0; o < 2; ++o) {   /* o=0 cart (dyn 0), o=1 pole (dyn 1) */
        dst[o * 7 + 0] = (float)S->x[o].x;
        dst[o * 7 + 1] = (float)S->x[o].y;
        dst[o * 7 + 2] = (float)S->x[o].z;
        for (int k = 0; k < 4; ++k) dst[o * 7 + 3 + k] = (float)S->q[o][k];
    }
}

int orc_envs_create(const cp_config* cfg, orc_envs** out) {
    /* the cp_create checks on the physics fields the oracle reads: NaN would silently
       turn the clamp off or keep bodies awake */
    if (!isfinite(cfg->phys.max_coord_velocity)) return -2;
    if ((cfg->phys.model_flags & CP_MODEL_SLEEPING) &&
        (!isfinite(cfg->phys.sleep_epsilon) || cfg->phys.sleep_epsilon < 0.0f ||
         !isfinite(cfg->phys.sleep_timeout) || cfg->phys.sleep_timeout < 0.0f))
        return -2;
    orc_envs* e = (orc_envs*)calloc(1, sizeof(orc_envs));
    if (!e) return -1;
    e->cfg = *cfg;
    e->B = cfg->num_envs;
    size_t B = (size_t)e->B;
    int R = cfg->action_repeats;
    e->state = calloc((size_t)CP_STATE_FIELDS * B, sizeof(real));
    e->term_obs = (float*)calloc((size_t)R * 14 * B, sizeof(float));
    e->bump_forces = (real*)calloc(B * (size_t)cfg->initial_force_steps * 4, sizeof(real));
    e->ret_acc = (float*)calloc(B, sizeof(float));
    e->last_ret = (float*)calloc(B, sizeof(float));
    e->last_len = (int32_t*)calloc(B, sizeof(int32_t));
    e->overflow = (int32_t*)calloc(B, sizeof(int32_t));
    e->nonfinite = (int32_t*)calloc(B, sizeof(int32_t));
    e->sweeps = (int32_t*)calloc((size_t)B * 2, sizeof(int32_t));
    e->merged = (int32_t*)calloc(B, sizeof(int32_t));
    e->pman = calloc(B * CP_NUM_PAIRS, sizeof(pman_t));
    if (cfg->autoreset == CP_AUTORESET_NEXT_STEP) e->held_obs = (float*)calloc((size_t)R * 14 * B, sizeof(float));
    for (int i = 0; i < e->B; ++i) {
        for (int d = 0; d < CP_NUM_DYN; ++d) {
            for (int k = 0; k < 3; ++k) SF(e, CP_SF_BODY(d, k), i) = cfg->phys.spawn_pos[d + 1][k];
            SF(e, CP_SF_BODY(d, 6), i) = 1.0f;
        }
        for (int p = 0; p < CP_NUM_ISLANDS; ++p)
            for (int j = 0; j < CP_ISLAND_PAIRS; ++j) set_i(e, CP_SF_WS_ID(p, j), i, -1);
        for (int d = 0; d < CP_NUM_DYN; ++d) set_i(e, CP_SF_SLEEP_ACT(d), i, CP_ACT_ACTIVE | CP_ACT_AWAKE);
        /* done = 1 until the first reset: step before reset is an error in the
         * reference (AttributeError); the batched API reports done. */
        set_i(e, CP_SF_DONE, i, 1);
    }
    *out = e;
    return 0;
}
void orc_envs_destroy(orc_envs* e) {
    if (!e) return;
    free(e->state); free(e->term_obs); free(e->bump_forces); free(e->ret_acc);
    free(e->last_ret); free(e->last_len); free(e->overflow); free(e->nonfinite); free(e->sweeps); free(e->merged); free(e->pman);
    free(e->held_obs);
    free(e);
}
/* cp_set_bump_forces / cp_set_bump_forces64: stored in the build's real type (widened exactly,
   or rounded to nearest) */
void orc_envs_set_bump_forces(orc_envs* e, const float* f) {
    const size_t n = (size_t)e->B * e->cfg.initial_force_steps * 4;
    for (size_t k = 0; k < n; ++k) ((real*)e->bump_forces)[k] = (real)f[k];
}
void orc_envs_set_bump_forces64(orc_envs* e, const double* f) {
    const size_t n = (size_t)e->B * e->cfg.initial_force_steps * 4;
    for (size_t k = 0; k < n; ++k) ((real*)e->bump_forces)[k] = (real)f[k];
}
void orc_envs_get_state(const orc_envs* e, void* out) {
    memcpy(out, e->state, (size_t)CP_STATE_FIELDS * e->B * sizeof(real));
}
void orc_envs_set_state(orc_envs* e, const void* in) {
    memcpy(e->state, in, (size_t)CP_STATE_FIELDS * e->B * sizeof(real));
    /* cp_set_state: the persistent manifolds (outside the state SoA) are cleared */
    memset(e->pman, 0, (size_t)e->B * CP_NUM_PAIRS * sizeof(pman_t));
}

/* bump force k (0..initial_force_steps-1) on cart c (0: cart, 1: cart2), LINK frame */
static void bump_force(const orc_envs* e, int i, int episode, int k, int c, real* fx, real* fy) {
    const cp_config* cfg = &e->cfg;
    if (cfg->bump_mode == CP_BUMP_HOST) {
        const real* f = (const real*)e->bump_forces + (((size_t)i * cfg->initial_force_steps + k) * 2 + c) * 2;
        *fx = f[0];
        *fy = f[1];
        return;
    }
    real F = (real)cfg->initial_force;
    if (!cfg->random_theta) { *fx = F; *fy = F * RC(0); return; }
    uint32_t idx = (uint32_t)(2 * k + c);
    uint64_t gid = (uint64_t)(cfg->env_id_offset + i);
    uint32_t ctr[4] = {idx >> 2, (uint32_t)episode, (uint32_t)gid, (uint32_t)(gid >> 32)};
    uint32_t key[2] = {(uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32)};
    uint32_t o[4];
    orc_philox4x32_10(ctr, key, o);
    real u = (real)(o[idx & 3] >> 8) * RC(5.9604644775390625e-08);
    real s, co;
    sincos_turns(u, &s, &co);
    *fx = F * co;
    *fy = F * s;
}

/* 1 if every body value (pos, quat, v, w of the 4 dynamic bodies) is finite (cp_nonfinite_counts) */
static int sim_finite(const sim_t* S) {
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        const real v[13] = {S->x[d].x, S->x[d].y, S->x[d].z, S->q[d][0], S->q[d][1], S->q[d][2], S->q[d][3],
                            S->v[d].x, S->v[d].y, S->v[d].z, S->w[d].x, S->w[d].y, S->w[d].z};
        for (int k = 0; k < 13; ++k)
            if (!isfinite(v[k])) return 0;
    }
    return 1;
}

static void reset_one(orc_envs* e, int i, float* obs_row /* R*14 */) {
    const cp_config* cfg = &e->cfg;
    sim_t S;
    env_load(e, i, &S);   /* keeps the pending forces (pybullet does not clear them) */
    if (cfg->reset_flags & CP_RESET_CLEAR_NONFINITE_FORCE)   /* opt-in: a NaN force does not outlive the reset */
        for (int c = 0; c < 2; ++c)
            if (!isfinite(S.f[2 * c].x) || !isfinite(S.f[2 * c].y) || !isfinite(S.f[2 * c].z))
                S.f[2 * c] = mk(RC(0), RC(0), RC(0));
    int episode = get_i(e, CP_SF_EPISODE, i);
    for (int d = 0; d < CP_NUM_DYN; ++d) {
        S.x[d] = mk((real)cfg->phys.spawn_pos[d + 1][0], (real)cfg->phys.spawn_pos[d + 1][1],
                    (real)cfg->phys.spawn_pos[d + 1][2]);
        S.q[d][0] = S.q[d][1] = S.q[d][2] = RC(0);
        S.q[d][3] = RC(1);
        S.v[d] = S.w[d] = mk(RC(0), RC(0), RC(0));
    }
    for (int p = 0; p < CP_NUM_ISLANDS; ++p)
        for (int j = 0; j < CP_ISLAND_PAIRS; ++j) {
            S.ws_id[p][j] = 0xFFFFFFFFu;
            for (int k = 0; k < 4; ++k) S.ws_lam[p][j][k] = RC(0);
            S.pm[p][j].cnt = 0;   /* resetBasePositionAndOrientation: no contact survives the teleport */
        }
    sleep_wake_all(&S);           /* CP_MODEL_SLEEPING: the teleported bodies are awake */
    int32_t ov = 0;
    for (int s = 0; s < cfg->settle_steps; ++s) substep(&S, &cfg->phys, &ov, NULL, NULL, NULL, NULL);
    for (int k = 0; k < cfg->initial_force_steps; ++k) {
        substep(&S, &cfg->phys, &ov, NULL, NULL, NULL, NULL);
        for (int c = 0; c < 2; ++c) {
            real fx, fy;
            bump_force(e, i, episode, k, c, &fx, &fy);
            apply_force_link(&S, 2 * c, fx, fy, RC(0));
        }
    }
    e->overflow[i] += ov;
    if (!sim_finite(&S)) e->nonfinite[i] += 1;
    env_store(e, i, &S);
    float row[14];
    write_obs_row(&S, row);
    for (int r = 0; r < cfg->action_repeats; ++r) memcpy(obs_row + r * 14, row, sizeof(row));
    set_i(e, CP_SF_STEPS, i, 0);
    set_i(e, CP_SF_DONE, i, 0);
    set_i(e, CP_SF_EPISODE, i, episode + 1);
    e->ret_acc[i] = 0.0f;
}

void orc_envs_reset(orc_envs* e, const uint8_t* mask, float* obs_out) {
    int R = e->cfg.action_repeats;
    for (int i = 0; i < e->B; ++i) {
        if (mask && !mask[i]) continue;
        if (e->cfg.autoreset == CP_AUTORESET_NEXT_STEP && get_i(e, CP_SF_DONE, i) >= 2) {
            /* its reset already ran (in the step that ended it): hand out that reset's obs */
            memcpy(obs_out + (size_t)i * R * 14, e->held_obs + (size_t)i * R * 14, (size_t)R * 14 * sizeof(float));
            set_i(e, CP_SF_DONE, i, 0);
            continue;
        }
        reset_one(e, i, obs_out + (size_t)i * R * 14);
    }
}

static const float DISCRETE_TABLE[CP_NUM_DISCRETE][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, 1}, {0, -1}};

static int bounds_exceeded(const orc_envs* e, const sim_t* S) {
    const cp_config* cfg = &e->cfg;
    v3 x = S->x[1];
    const real* q = S->q[1];
    if (FABS(x.x) > (real)cfg->pos_threshold || FABS(x.y) > (real)cfg->pos_threshold) return 1;
    real qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    real Y = RC(2) * FMA(qy, qz, qw * qx);
    real X = ((qw * qw - qx * qx) - qy * qy) + qz * qz;
    int roll_out = (X > RC(0)) ? (FABS(Y) > X * (real)cfg->tan_angle_threshold) : !(X == RC(0) && Y == RC(0));
    real sarg = RC(-2) * FMA(qx, qz, -(qw * qy));
    int pitch_out = FABS(sarg) > (real)cfg->sin_angle_threshold;
    return roll_out || pitch_out;
}

static void readback_pole(const sim_t* S, int pole_dyn, int vel_dyn, float* dst /* 12 */) {
    real rpy[3];
    quat_euler(S->q[pole_dyn], rpy);
    dst[0] = (float)S->x[pole_dyn].x; dst[1] = (float)S->x[pole_dyn].y; dst[2] = (float)S->x[pole_dyn].z;
    dst[3] = (float)rpy[0]; dst[4] = (float)rpy[1]; dst[5] = (float)rpy[2];
    dst[6] = (float)S->v[vel_dyn].x; dst[7] = (float)S->v[vel_dyn].y; dst[8] = (float)S->v[vel_dyn].z;
    dst[9] = (float)S->w[vel_dyn].x; dst[10] = (float)S->w[vel_dyn].y; dst[11] = (float)S->w[vel_dyn].z;
}

/* ---- LQR policy (random_action_agent.py:60-135; cp_kernels.hip lqr_*) ---- */
void orc_envs_set_lqr(orc_envs* e, const float* gains, int per_env, float* state8_out, float done_pos,
                      float done_angle) {
    e->lqr_gains = gains;
    e->lqr_per_env = per_env ? 1 : 0;
    e->lqr_state8 = state8_out;
    e->lqr_done_pos = done_pos;
    e->lqr_done_angle = done_angle;
}

/* pole 8-state (:121-135): x - x0, x', y, y', roll, roll', pitch, pitch' */
static void pole_state8(const sim_t* S, int pole_dyn, real x0, real s[8]) {
    real rpy[3];
    quat_euler(S->q[pole_dyn], rpy);
    s[0] = S->x[pole_dyn].x - x0; s[1] = S->v[pole_dyn].x; s[2] = S->x[pole_dyn].y; s[3] = S->v[pole_dyn].y;
    s[4] = rpy[0]; s[5] = S->w[pole_dyn].x; s[6] = rpy[1]; s[7] = S->w[pole_dyn].y;
}

/* u = -K s (:92-95) for both pairs; returns 1 when both pairs are out of bounds (:108-119, :908) */
static int lqr_observe(const orc_envs* e, const sim_t* S, const float* K, real u[2][2], float* s8_out) {
    int out[2];
    for (int p = 0; p < 2; ++p) {
        real s[8];
        const int pole = 2 * p + 1;
        pole_state8(S, pole, (real)e->cfg.phys.spawn_pos[pole + 1][0], s);
        if (s8_out)
            for (int k = 0; k < 8; ++k) s8_out[8 * p + k] = (float)s[k];
        real ax = RC(0), ay = RC(0);
        for (int k = 0; k < 8; ++k) {
            ax = FMA((real)K[16 * p + k], s[k], ax);
            ay = FMA((real)K[16 * p + 8 + k], s[k], ay);
        }
        u[p][0] = -ax;
        u[p][1] = -ay;
        const real pos = (real)e->lqr_done_pos, ang = (real)e->lqr_done_angle;
        out[p] = FABS(s[0]) > pos || FABS(s[2]) > pos || FABS(s[4]) > ang || FABS(s[6]) > ang;
    }
    return e->lqr_done_pos > 0.0f && out[0] && out[1];
}

static void step_one(orc_envs* e, int i, const void* actions, int kind, float* obs_out, float* reward_out,
                     uint8_t* done_out, float* term_out, float* readback, int rb_bug, int par) {
    const cp_config* cfg = &e->cfg;
    const int R = cfg->action_repeats, Sn = cfg->steps_per_repeat;
    float* obs = obs_out + (size_t)i * R * 14;
    if (cfg->autoreset == CP_AUTORESET_NEXT_STEP && get_i(e, CP_SF_DONE, i) >= 2) {
        /* ended in the previous step: the new episode's first obs, reward 0, done 0; action ignored */
        memcpy(obs, e->held_obs + (size_t)i * R * 14, (size_t)R * 14 * sizeof(float));
        reward_out[i] = 0.0f;
        done_out[i] = 0;
        set_i(e, CP_SF_DONE, i, 0);
        return;
    }
    if (get_i(e, CP_SF_DONE, i)) {     /* bullet_cartpole.py:179-181 */
        for (int f = 0; f < R * 14; ++f) obs[f] = e->term_obs[(size_t)f * e->B + i];
        reward_out[i] = 0.0f;
        done_out[i] = 1;
        return;
    }
    real a[2][2];
    if (kind == CP_ACTION_CONTINUOUS) {
        const float* A = (const float*)actions + (size_t)i * 4;
        a[0][0] = A[0]; a[0][1] = A[1]; a[1][0] = A[2]; a[1][1] = A[3];
    } else {
        const int8_t* A = (const int8_t*)actions + (size_t)i * 2;
        for (int c = 0; c < 2; ++c) {
            int k = A[c];
            if (k < 0 || k >= CP_NUM_DISCRETE) k = 0;
            a[c][0] = DISCRETE_TABLE[k][0];
            a[c][1] = DISCRETE_TABLE[k][1];
        }
    }
    const real F = (real)cfg->action_force;
    sim_t S;
    env_load(e, i, &S);
    int32_t ov = 0;
    int32_t* sw = e->sweeps + (size_t)i * 2;
    sw[0] = sw[1] = 0;
    e->merged[i] = 0;
    real u[2][2] = {{RC(0), RC(0)}, {RC(0), RC(0)}};
    int lqr_done = 0;
    const float* K = e->lqr_gains ? e->lqr_gains + (e->lqr_per_env ? (size_t)i * 32 : 0) : NULL;
    if (K) lqr_observe(e, &S, K, u, NULL);
    for (int r = 0; r < R; ++r) {
        for (int s = 0; s < Sn; ++s) {
            substep(&S, &cfg->phys, &ov, NULL, NULL, sw, &e->merged[i]);
            if (K) {   /* disturbance + control from the pre-step state (:897-901) */
                apply_force_link(&S, 0, a[0][0] * F + u[0][0], a[0][1] * F + u[0][1], RC(0));
                apply_force_link(&S, 2, a[1][0] * F + u[1][0], a[1][1] * F + u[1][1], RC(0));
                float* s8 = e->lqr_state8 ? e->lqr_state8 + (((size_t)i * R + r) * Sn + s) * 16 : NULL;
                lqr_done |= lqr_observe(e, &S, K, u, s8);
            } else {
                apply_force_link(&S, 0, a[0][0] * F, a[0][1] * F, RC(0));
                apply_force_link(&S, 2, a[1][0] * F, a[1][1] * F, RC(0));
            }
            if (readback) {
                size_t base = (size_t)i * 2 * R * Sn * 12;
                readback_pole(&S, 1, 1, readback + base + ((size_t)(0 * R + r) * Sn + s) * 12);
                readback_pole(&S, 3, rb_bug ? 1 : 3, readback + base + ((size_t)(1 * R + r) * Sn + s) * 12);
            }
        }
        write_obs_row(&S, obs + r * 14);
    }
    e->overflow[i] += ov;
    int steps = get_i(e, CP_SF_STEPS, i) + 1;
    int done = steps >= cfg->max_episode_len;
    if (cfg->done_on_bounds && bounds_exceeded(e, &S)) done = 1;
    if (lqr_done) done = 1;
    if (!sim_finite(&S)) e->nonfinite[i] += 1;
    env_store(e, i, &S);
    set_i(e, CP_SF_STEPS, i, steps);
    reward_out[i] = 1.0f;            /* bullet_cartpole.py:260 */
    done_out[i] = (uint8_t)done;
    e->ret_acc[i] += 1.0f;
    if (done) {
        e->last_ret[i] = e->ret_acc[i];
        e->last_len[i] = steps;
        e->ret_acc[i] = 0.0f;
        for (int f = 0; f < R * 14; ++f) e->term_obs[(size_t)f * e->B + i] = obs[f];
        if (term_out) memcpy(term_out + (size_t)i * R * 14, obs, (size_t)R * 14 * sizeof(float));
        set_i(e, CP_SF_DONE, i, 1);
        if (cfg->autoreset == CP_AUTORESET_NEXT_STEP) {
            reset_one(e, i, e->held_obs + (size_t)i * R * 14);
            set_i(e, CP_SF_DONE, i, 2 + par);
        } else if (cfg->autoreset) {
            reset_one(e, i, obs);
        }
    }
}

/* the parity of this step (CP_AUTORESET_NEXT_STEP's done code); toggles per step call */
static int next_par(orc_envs* e) {
    const int q = e->npar;
    e->npar ^= 1;
    return q;
}
void orc_envs_step(orc_envs* e, const void* actions, int kind, float* obs_out, float* reward_out,
                   uint8_t* done_out, float* term_out, float* readback, int rb_bug) {
    const int q = next_par(e);
    for (int i = 0; i < e->B; ++i)
        step_one(e, i, actions, kind, obs_out, reward_out, done_out, term_out, readback, rb_bug, q);
}
void orc_envs_step_range(orc_envs* e, int lo, int hi, const void* actions, int kind, float* obs_out,
                         float* reward_out, uint8_t* done_out) {
    /* a shard of one step: NEXT_STEP handles step through orc_envs_step */
    for (int i = lo; i < hi; ++i) step_one(e, i, actions, kind, obs_out, reward_out, done_out, NULL, NULL, 0, 0);
}
int orc_envs_step_omp(orc_envs* e, const void* actions, int kind, float* obs_out, float* reward_out,
                      uint8_t* done_out, int threads) {
    int used = 1;
    const int q = next_par(e);
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel
    {
#pragma omp single
        used = omp_get_num_threads();
#pragma omp for schedule(static)
        for (int i = 0; i < e->B; ++i)
            step_one(e, i, actions, kind, obs_out, reward_out, done_out, NULL, NULL, 0, q);
    }
#else
    (void)threads;
    for (int i = 0; i < e->B; ++i) step_one(e, i, actions, kind, obs_out, reward_out, done_out, NULL, NULL, 0, q);
#endif
    return used;
}
void orc_envs_sweeps(const orc_envs* e, int32_t* out) { memcpy(out, e->sweeps, (size_t)e->B * 2 * sizeof(int32_t)); }
void orc_envs_nonfinite(const orc_envs* e, int32_t* out) { memcpy(out, e->nonfinite, (size_t)e->B * sizeof(int32_t)); }
void orc_envs_overflow(const orc_envs* e, int32_t* out) { memcpy(out, e->overflow, (size_t)e->B * sizeof(int32_t)); }
void orc_envs_merged(const orc_envs* e, int32_t* out) { memcpy(out, e->merged, (size_t)e->B * sizeof(int32_t)); }
void orc_envs_episode_returns(const orc_envs* e, float* ret, int32_t* len) {
    if (ret) memcpy(ret, e->last_ret, (size_t)e->B * sizeof(float));
    if (len) memcpy(len, e->last_len, (size_t)e->B * sizeof(int32_t));
}
