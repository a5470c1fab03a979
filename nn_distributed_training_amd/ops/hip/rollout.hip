// On-device rollout of the multi-agent PPO tree (rl/device_rollout.py):
// one block runs one whole episode of rl/envs.py SimpleTagEnv with every
// node's actor, and writes the batch straight into the [N*M, .] layout
// of rl/stacked_ppo.py StackedPPOEngine.
//
// An episode of this env ends only at its step limit, so episode e of a
// batch of M steps covers rows [e*ep_len, e*ep_len + len_e),
// len_e = min(ep_len, M - e*ep_len), known before the launch; episodes
// depend only on their reset positions and action noise.
//
// Per step (tid = node * W + unit, W = widest layer of the actor):
//   A  observations of all N predators from the state (the layout of
//      SimpleTagEnv._observations), cast to T, to LDS and to obs[];
//      the last thread computes the previous step's reward
//   B  actor MLP, one thread per (node, output unit), activations
//      ping-pong between two LDS buffers, one barrier per layer
//   C  act = mean + sqrt(cov) * eps, logp = -|eps|^2/2 - logc
//   D  one thread per movable entity: action force (the prey's from
//      the reference evader heuristic), contact forces against every
//      other entity and obstacle in the order SimpleTagEnv._forces adds
//      them, MPE integrator; the new state goes to the other state
//      buffer, so one barrier ends the step
// and after the last step a serial reverse scan gives the rewards-to-go.
// With last_obs ([N*E, obs_dim], row l*E + e) the block also writes the
// observation of the state its last step left, phase A's formula
// (obs_element) once more: what env.step returned at the episode's end,
// for partial-episode bootstrapping (rl/advantages.py).
// The env state and all env arithmetic are double for either T: the
// host env is double and casts only the observation.
//
// The grid is E blocks (6 at the default shape), each a serial chain of
// ep_len dependent steps: latency-bound by construction, occupancy is
// not the lever. WLDS stages all actors' weights in LDS once per block
// (they are re-read every step); without it they are read in place from
// the [N, n] stack, which stays L2-resident. A thread's dot product
// starts at column (unit mod I) and wraps, so the lanes of a wave read
// distinct LDS banks of a row-major weight matrix.

#include "common.h"

namespace rollout {

constexpr int MAX_N = 8;        // predators (= graph nodes)
constexpr int MAX_OBST = 8;     // SimpleTagEnv's obstacle table
constexpr int MAX_LAYERS = 8;
constexpr int MAX_W = 128;      // widest activation row, obs included
constexpr int ACT_DIM = 5;      // MPE force parameterization

// the actor's layers at the offsets of shifted_plan(actors[0], 0)
struct Plan {
  int nl;
  int in_dim[MAX_LAYERS], out_dim[MAX_LAYERS];
  int w_off[MAX_LAYERS], b_off[MAX_LAYERS];
  int relu[MAX_LAYERS];
};

// SimpleTagEnv's constants (attributes of the env and of rl/envs.py)
struct EnvParams {
  double pred_size, prey_size, obst_size;
  double pred_accel, prey_accel, pred_vmax, prey_vmax;
  double dt, damping, margin, contact;
};

// rl/envs.py mpe_collision_force for delta = (dx, dy)
DEV_INLINE void contact_force(double dx, double dy, double dist_min,
                              const EnvParams& p, double& fx,
                              double& fy) {
  const double dist = ::sqrt(dx * dx + dy * dy);
  // logaddexp(0, v), as numpy evaluates it
  const double v = -(dist - dist_min) / p.margin;
  const double la =
      v < 0.0 ? ::log1p(::exp(v)) : v + ::log1p(::exp(-v));
  const double pen = la * p.margin;
  const double dm = dist > 1e-12 ? dist : 1e-12;
  fx = p.contact * dx / dm * pen;
  fy = p.contact * dy / dm * pen;
}

// SimpleTagEnv._rewards on the state a step left: the MPE adversary
// team reward, the same for every predator
DEV_INLINE double team_reward(const double (*pos)[2], int N,
                              const EnvParams& p) {
  double dsum = 0.0;
  int ncoll = 0;
  for (int j = 0; j < N; ++j) {
    const double dx = pos[j][0] - pos[N][0];
    const double dy = pos[j][1] - pos[N][1];
    const double dj = ::sqrt(dx * dx + dy * dy);
    dsum += dj;
    ncoll += dj < p.pred_size + p.prey_size ? 1 : 0;
  }
  return -0.1 * dsum + 10.0 * ncoll;
}

// Element c of predator i's observation in the state (pos, vel): the
// layout of SimpleTagEnv._observations
DEV_INLINE double obs_element(const double (*pos)[2],
                              const double (*vel)[2], int N, int i,
                              int c) {
  const int d = c & 1;
  if (c < 2) return vel[i][d];
  if (c < 4) return pos[i][d];
  if (c < 2 * N + 2) {
    const int k = (c - 4) >> 1;
    const int j = k < i ? k : k + 1;  // world order, self skipped
    return pos[j][d] - pos[i][d];
  }
  if (c < 2 * N + 4) return pos[N][d] - pos[i][d];
  return vel[N][d];
}

template <typename T, bool WLDS>
__global__ void ppo_rollout_k(
    const T* __restrict__ theta, long n, Plan plan, int span, int W,
    const double* __restrict__ resets,  // [E, N+1, 2]
    const double* __restrict__ obst,    // [n_obst, 2]
    const T* __restrict__ eps,          // [E, ep_len, N, ACT_DIM]
    T* __restrict__ obs,                // [N*M, obs_dim]
    T* __restrict__ acts,               // [N*M, ACT_DIM]
    T* __restrict__ logp,               // [N*M]
    double* __restrict__ rews,          // [M]
    T* __restrict__ rtgs,               // [N*M]
    double* __restrict__ ep_rew,        // [E]
    int N, int n_obst, int M, int ep_len, T sd, T logc, double gamma,
    EnvParams env,
    T* __restrict__ last_obs) {         // [N*E, obs_dim], may be null
  __shared__ double s_pos[2][MAX_N + 1][2];
  __shared__ double s_vel[2][MAX_N + 1][2];
  __shared__ double s_obst[MAX_OBST][2];
  __shared__ double s_act[MAX_N][ACT_DIM];
  __shared__ T s_x[2][MAX_N][MAX_W];
  extern __shared__ __align__(16) unsigned char rollout_raw[];
  double* s_rew = reinterpret_cast<double*>(rollout_raw);  // [ep_len]
  T* s_w = reinterpret_cast<T*>(s_rew + ep_len);           // [N, span]

  const int tid = threadIdx.x;
  const int e = blockIdx.x;
  const int base = e * ep_len;
  const int len = ep_len < M - base ? ep_len : M - base;
  const int obs_dim = 2 * N + 6;
  const int node = tid / W, unit = tid - node * W;
  const int rew_tid = blockDim.x - 1;  // > N * obs_dim (launcher)

  if (tid < 2 * (N + 1)) {
    const int ent = tid >> 1, d = tid & 1;
    s_pos[0][ent][d] = resets[((long)e * (N + 1) + ent) * 2 + d];
    s_vel[0][ent][d] = 0.0;
  }
  if (tid < 2 * n_obst) s_obst[tid >> 1][tid & 1] = obst[tid];
  if (WLDS) {
    for (int i = tid; i < N * span; i += blockDim.x) {
      const int l = i / span;
      s_w[i] = theta[l * n + (i - l * span)];
    }
  }
  const T* wbase = WLDS ? s_w + node * span : theta + node * n;
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < len; ++t) {
    const long row0 = base + t;
    // ---- A: observations, and the reward of the step before
    if (tid < N * obs_dim) {
      const int i = tid / obs_dim, c = tid - i * obs_dim;
      const double o = obs_element(s_pos[cur], s_vel[cur], N, i, c);
      s_x[0][i][c] = (T)o;
      obs[((long)i * M + row0) * obs_dim + c] = (T)o;
    }
    if (tid == rew_tid && t > 0) {
      const double r = team_reward(s_pos[cur], N, env);
      s_rew[t - 1] = r;
      rews[row0 - 1] = r;
    }
    __syncthreads();

    // ---- B: actor forward
    int xb = 0;
    for (int li = 0; li < plan.nl; ++li) {
      const int I = plan.in_dim[li], O = plan.out_dim[li];
      if (node < N && unit < O) {
        const T* w = wbase + plan.w_off[li] + unit * I;
        const T* x = s_x[xb][node];
        T acc = wbase[plan.b_off[li] + unit];
        int k = unit % I;
        for (int c = 0; c < I; ++c) {
          acc += w[k] * x[k];
          k = k + 1 == I ? 0 : k + 1;
        }
        if (plan.relu[li]) acc = acc > T(0) ? acc : T(0);
        s_x[xb ^ 1][node][unit] = acc;
      }
      __syncthreads();
      xb ^= 1;
    }

    // ---- C: Gaussian action and its log-probability
    if (tid < N * ACT_DIM) {
      const int i = tid / ACT_DIM, j = tid - i * ACT_DIM;
      const T* ep = eps + (((long)e * ep_len + t) * N + i) * ACT_DIM;
      const T a = s_x[xb][i][j] + sd * ep[j];
      acts[((long)i * M + row0) * ACT_DIM + j] = a;
      s_act[i][j] = (double)a;
      if (j == 0) {
        T sq = T(0);
#pragma unroll
        for (int q = 0; q < ACT_DIM; ++q) sq += ep[q] * ep[q];
        logp[(long)i * M + row0] = T(-0.5) * sq - logc;
      }
    }
    __syncthreads();

    // ---- D: SimpleTagEnv.step, one thread per movable entity
    if (tid <= N) {
      const int me = tid;
      const bool prey = me == N;
      const double px = s_pos[cur][me][0], py = s_pos[cur][me][1];
      double ux, uy;
      if (!prey) {
        ux = s_act[me][1] - s_act[me][2];
        uy = s_act[me][3] - s_act[me][4];
      } else {
        // _prey_heuristic_action: flee the nearest predator (first
        // minimum), force normalized by its max |component|, outward
        // channel zeroed at the +-1.2 boundary
        double best = 0.0, nx = 0.0, ny = 0.0;
        for (int j = 0; j < N; ++j) {
          const double dx = s_pos[cur][j][0] - px;
          const double dy = s_pos[cur][j][1] - py;
          const double dj = ::sqrt(dx * dx + dy * dy);
          if (j == 0 || dj < best) {
            best = dj; nx = dx; ny = dy;
          }
        }
        const double ax = nx < 0.0 ? -nx : nx, ay = ny < 0.0 ? -ny : ny;
        double mx = ax > ay ? ax : ay;
        mx = mx > 1e-12 ? mx : 1e-12;
        ux = -nx / mx;
        uy = -ny / mx;
        if (px <= -1.2) ux = ux > 0.0 ? ux : 0.0;
        else if (px >= 1.2) ux = ux > 0.0 ? 0.0 : ux;
        if (py <= -1.2) uy = uy > 0.0 ? uy : 0.0;
        else if (py >= 1.2) uy = uy > 0.0 ? 0.0 : uy;
      }
      const double accel = prey ? env.prey_accel : env.pred_accel;
      const double size = prey ? env.prey_size : env.pred_size;
      const double vmax = prey ? env.prey_vmax : env.pred_vmax;
      double fx = ux * accel, fy = uy * accel;
      for (int b = 0; b <= N; ++b) {
        if (b == me) continue;
        // the pair's force is computed as for its lower index a, at
        // +delta from b, and subtracted on b's side, as _forces does
        const int lo = b < me ? b : me, hi = b < me ? me : b;
        const double sb = b == N ? env.prey_size : env.pred_size;
        double cx, cy;
        contact_force(s_pos[cur][lo][0] - s_pos[cur][hi][0],
                      s_pos[cur][lo][1] - s_pos[cur][hi][1], size + sb,
                      env, cx, cy);
        if (me == lo) {
          fx += cx; fy += cy;
        } else {
          fx -= cx; fy -= cy;
        }
      }
      for (int o = 0; o < n_obst; ++o) {
        double cx, cy;
        contact_force(px - s_obst[o][0], py - s_obst[o][1],
                      size + env.obst_size, env, cx, cy);
        fx += cx; fy += cy;
      }
      // MPE integrator: damp, accelerate, clamp the speed, move
      double vx = s_vel[cur][me][0] * (1.0 - env.damping) + fx * env.dt;
      double vy = s_vel[cur][me][1] * (1.0 - env.damping) + fy * env.dt;
      const double sp = ::sqrt(vx * vx + vy * vy);
      if (sp > vmax) {
        vx = vx / sp * vmax;
        vy = vy / sp * vmax;
      }
      s_vel[cur ^ 1][me][0] = vx;
      s_vel[cur ^ 1][me][1] = vy;
      s_pos[cur ^ 1][me][0] = px + vx * env.dt;
      s_pos[cur ^ 1][me][1] = py + vy * env.dt;
    }
    __syncthreads();
    cur ^= 1;
  }

  // the observation the env returns after the episode's last step (the
  // cut episode's too), for a caller that bootstraps truncated ends
  if (last_obs != nullptr && tid < N * obs_dim) {
    const int i = tid / obs_dim, c = tid - i * obs_dim;
    const long E = gridDim.x;
    last_obs[((long)i * E + e) * obs_dim + c] =
        (T)obs_element(s_pos[cur], s_vel[cur], N, i, c);
  }
  // the last step's reward, then rewards-to-go and the episode's sum
  if (tid == 0) {
    const double r = team_reward(s_pos[cur], N, env);
    s_rew[len - 1] = r;
    rews[base + len - 1] = r;
    double sum = 0.0;
    for (int t = 0; t < len; ++t) sum += s_rew[t];
    ep_rew[e] = sum;
    double run = 0.0;
    for (int t = len - 1; t >= 0; --t) {
      run = s_rew[t] + gamma * run;
      s_rew[t] = run;
    }
  }
  __syncthreads();
  for (int i = tid; i < N * len; i += blockDim.x) {
    const int l = i / len, t = i - l * len;
    rtgs[(long)l * M + base + t] = (T)s_rew[t];
  }
}

}  // namespace rollout
