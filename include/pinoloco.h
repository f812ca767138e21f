/*
 * pinoloco -- C-ABI of the MI355X-native batched MPC inner loop.
 *
 * Drop-in boundary for the reference's OSQP-SQP solve path
 * (lukasmolnar/pino-locoman @ 2025-05-09).  Each entry point replaces a
 * reference interface, cited as file:line of the reference:
 *
 *   pl_model_create       <- RobotWrapper.BuildFromURDF + buildReducedRobot
 *                            (utils/robot.py:13-22); the host parser
 *                            pinoloco/model.py produces the tables.
 *   pl_ocp_create         <- make_ocp(dynamics, OCP_ARGS, robot, nodes, solver)
 *                            (optimization/ocp_factory.py:8-27) + setup_problem
 *                            (optimization/ocp.py:38-44): variable/row layout and
 *                            the Jacobian sparsity of J_g (ocp.py:283, 305).
 *   pl_ocp_set_params     <- opti.set_value(...) of every parameter
 *                            (ocp.py:216-242, ocp_whole_body_rnea.py:204); the
 *                            array is opti.p in declaration order (ocp.py:54-69).
 *   pl_ocp_set_x          <- opti.set_initial(...) / warm_start()
 *                            (ocp.py:161-163, ocp_whole_body_rnea.py:207-235).
 *   pl_ocp_init_solver    <- OCP.init_solver() OSQP branch (ocp.py:265-313):
 *                            constant Hessian diagonal, OSQP setup.
 *   pl_ocp_solve          <- OCP.solve() OSQP branch minus retract
 *                            (ocp.py:375-414): sqp_data, osqp.update/solve,
 *                            _armijo_line_search, max violation.
 *   pl_eval_sqp_data      <- the CasADi Function sqp_data(x, p) ->
 *                            (grad_f, J_g, g, lbg, ubg) (ocp.py:287, 386).
 *   pl_eval_f             <- f_data (ocp.py:289); g_data is the g/lbg/ubg part
 *                            of pl_eval_sqp_data (ocp.py:290).
 *   pl_mpc_*              <- run_mpc.mpc_loop OSQP branch (run_mpc.py:115-143)
 *                            executed on the device for a whole batch.
 *
 * Conventions: all host arrays are caller-owned, C-contiguous float64,
 * problem-major ([batch][len]).  The library copies them into device buffers
 * it owns.  Functions return 0 on success and a negative value on error; the
 * message is available from pl_last_error() (thread-local).  Per-problem
 * solver failures are reported in pl_stats.status, never as a call failure.
 * A handle is bound to one HIP device and stream and is not thread-safe.
 * Calls are synchronous with respect to host buffers on return.
 */
#ifndef PINOLOCO_H_
#define PINOLOCO_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pl_model pl_model;
typedef struct pl_ocp pl_ocp;

/* Joint types (JointModelFreeFlyer root + revolute joints, utils/robot.py:14). */
#define PL_JOINT_FREEFLYER 1
#define PL_JOINT_REVOLUTE 2

/* Dynamics kinds (ocp_factory.py:9-15). */
#define PL_DYN_WHOLE_BODY_RNEA 0
#define PL_DYN_WHOLE_BODY_ACC 1
#define PL_DYN_WHOLE_BODY_ABA 2
#define PL_DYN_CENTROIDAL_VEL 3      /* x = [h (6), q], dx = [dh, dq], u = [v | f] */
#define PL_DYN_CENTROIDAL_ACC 4      /* x = [q, v], u = [a | f] (include_base) or [a_j | f] */

typedef struct {
  int njoints;                 /* including the universe joint 0 */
  int nq, nv;
  const int* parent;           /* [njoints] */
  const int* jtype;            /* [njoints] PL_JOINT_* (0 for universe) */
  const double* axis;          /* [njoints*3] revolute axis in the joint frame */
  const double* placement_R;   /* [njoints*9] jointPlacement rotation (row-major) */
  const double* placement_p;   /* [njoints*3] */
  const double* mass;          /* [njoints] body inertias (fixed children merged) */
  const double* lever;         /* [njoints*3] CoM in the joint frame */
  const double* inertia;       /* [njoints*9] rotational inertia at the CoM */
  const double* gravity;       /* [3] */
  int nframes;
  const int* frame_parent;     /* [nframes] parent joint */
  const double* frame_R;       /* [nframes*9] placement w.r.t. the parent joint */
  const double* frame_p;       /* [nframes*3] */
} pl_model_desc;

typedef struct {
  int dynamics;                /* PL_DYN_* */
  int nodes;                   /* N */
  int tau_nodes;               /* OCP_ARGS["whole_body_rnea"]["tau_nodes"] (ocp_args.py:16) */
  int include_acc;             /* rnea: 1 = a in u (ocp_args.py:17), 0 = a = (v_{i+1} - v_i) / dt (ocp_whole_body_rnea.py:183-191; OSQP branch only) */
  int include_base;            /* acc / centroidal_acc / centroidal_vel: 1 = base in u (ocp_args.py:5-11);
                                  0 = base acceleration / velocity from the dynamics
                                  (ocp_whole_body_acc.py:124-135, ocp_centroidal_vel.py:119-129) */
  int n_feet;                  /* 4: FR, FL, RR, RL (utils/gait_sequence.py:7) */
  int foot_frames[4];
  int ext_force_frame;         /* -1: none */
  int arm_ee_frame;            /* -1: none */
  int base_frame;              /* "base_link" frame, -1 if absent (dynamics/dynamics.py:17) */
  double mu;                   /* friction coefficient 0.7 (ocp.py:103) */
  const double* q0;            /* [nq] reference pose (SRDF) */
  const double* joint_pos_min; /* [nj] */
  const double* joint_pos_max;
  const double* joint_vel_max;
  const double* joint_torque_max;
  /* OSQP settings (ocp.py:267-273 + OSQP 0.6 defaults) */
  double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int max_iter, scaling, check_termination, warm_start;
  /* gait used by the device-side MPC loop (utils/gait_sequence.py:5-24) */
  int gait_type;               /* 0 trot, 1 walk, 2 stand */
  double gait_period;
  /* 0 in production.  Bits of PL_PATH_*: the paths earlier builds used, kept as the references
     the regression tests compare the current kernels with (tests/test_r04_paths.py,
     tests/test_qp_kernels.py, tests/test_graph_gpu.py), and the phase-timing instrumentation.
     No environment variable changes a kernel path; pl_ocp_sizes reports this field.
     Callers must zero-initialise the struct: pl_ocp_create rejects bits outside PL_PATH_ALL. */
  unsigned debug_paths;
} pl_ocp_desc;

#define PL_PATH_JAC_DUAL_ALL    1u   /* rnea a / f Jacobian columns as dual lanes (not k_eval_jac_lin) */
#define PL_PATH_JAC_CONST_EVERY 2u   /* the constant Jacobian columns re-evaluated every time */
#define PL_PATH_HESS_FULL_TREE  4u   /* Lagrangian-Hessian passes over the whole tree (no chain confinement) */
#define PL_PATH_HESS_DUAL_ALL   8u   /* the (dq, a) / (dq, f) Hessian blocks as hyper-dual pairs */
#define PL_PATH_FCHAIN_LIST     16u  /* the factor chain's E_{i+1} by list sums (not the f64 MFMA) */
#define PL_PATH_RUIZ_PER_PASS   32u  /* Ruiz equilibration as per-pass kernels (not k_ruiz_fused) */
#define PL_PATH_NO_MPC_GRAPH    64u  /* pl_mpc_step launches eagerly (no HIP graph) */
#define PL_PATH_ADMM_TIMING     128u /* s_memtime phase timing in the sweep / factor kernels (pl_debug_get "admm_t") */
#define PL_PATH_IP_REFINE_GATHER 256u /* k_ip_refine's H_i dx by the per-column global gather (the nw > 192 path) */
#define PL_PATH_HESS_PAIRS      512u /* the (dq, dq) / (dq, dv) Hessian pairs by one hyper-dual sweep each (r05), not
                                        the forward-over-reverse columns */
#define PL_PATH_RC_ONE_GROUP    1024u /* the chain ADMM kernel on one workgroup per problem (r05), not the
                                         multi-workgroup node phases */
#define PL_PATH_ALL             2047u /* pl_ocp_create rejects any other bit: callers zero the struct */

typedef struct {
  int status;                  /* OSQP status code (1 solved, 2 inaccurate, -2 max iter, ...) */
  int admm_iters;
  int ls_accepted;             /* line search accepted a step (ocp.py:473-480) */
  int ls_branch;               /* 1: g high & improving, 2: armijo, 3: filter */
  int ls_trials;
  int pad;
  double ls_alpha;             /* accepted step length (a / a_decay, ocp.py:475) */
  double viol_max;             /* _constraint_violation_max after the step (ocp.py:412-414) */
  double pri_res, dua_res;
  double f;                    /* objective at the returned point */
} pl_stats;

const char* pl_last_error(void);
int pl_version(void);
/* "pl_src_sha256=<hex> arch=gfx950": the sha256 of the csrc/ and include/ sources this
   library was built from (pinoloco/build.py source_sha). */
const char* pl_build_info(void);

int pl_model_create(const pl_model_desc* desc, pl_model** out);
void pl_model_destroy(pl_model* m);

/* device = -1 builds a host-only handle (layout/pattern queries, no solves). */
int pl_ocp_create(const pl_model* model, const pl_ocp_desc* desc, int batch, int device, pl_ocp** out);
void pl_ocp_destroy(pl_ocp* o);

/* n decision variables, m rows, np parameters, nnz Jacobian entries. */
int pl_ocp_dims(const pl_ocp* o, int* n, int* m, int* np, int* nnz);
/* Jacobian pattern in the library's entry order: global (row, col) per entry. */
int pl_ocp_pattern(const pl_ocp* o, int* rows, int* cols);

int pl_ocp_set_params(pl_ocp* o, const double* P);   /* [batch][np] */
int pl_ocp_get_params(pl_ocp* o, double* P);
int pl_ocp_set_x(pl_ocp* o, const double* X);        /* [batch][n] */
int pl_ocp_get_x(pl_ocp* o, double* X);
int pl_ocp_init_solver(pl_ocp* o);                   /* Hessian diag + reset ADMM iterates */
/* One SQP iteration in place for the whole batch.  stats: [batch] or NULL;
 * phase_ms: [4] (data, update+factor, admm, line search) or NULL. */
int pl_ocp_solve(pl_ocp* o, pl_stats* stats, double* phase_ms);
/* SQP iterations per pl_ocp_solve / pl_mpc_step (default 1 = the reference's
 * `for _ in range(1)`, optimization/ocp.py:382-383). */
int pl_ocp_set_sqp_iters(pl_ocp* o, int sqp_iters);

/* Interior-point solve: the reference's Fatrop branch (ocp.py:248-263 settings,
 * :360-373 solve; run_mpc.py:34-37 selects it), restated as an IPOPT-style
 * primal-dual barrier method with a filter line search (oracle/ip_ref.py documents
 * the algorithm).  pl_ocp_set_solver(o, PL_SOLVER_IP) switches pl_ocp_solve and
 * pl_mpc_step to it; pl_stats then holds status (1 converged, -1 max_iter, -2 line
 * search failed, -3 non-finite), admm_iters = IP iterations, ls_trials (total),
 * ls_alpha (last step), viol_max, pri_res = scaled NLP error, dua_res = mu, f. */
#define PL_SOLVER_OSQP 0
#define PL_SOLVER_IP 1
typedef struct {
  double tol;          /* 1e-3  (ocp.py:257) */
  double mu_init;      /* 1e-4  (ocp.py:258) */
  double bound_push;   /* 1e-7  (ocp.py:261) */
  double bound_frac;   /* 1e-2 */
  double delta_w;      /* 1e-8  primal regularisation of the Newton system */
  double delta_c;      /* 1e-4  dual regularisation (equality rows weighted 1 / delta_c) */
  int max_iter;        /* 10    (ocp.py:256), at most 32 */
  int ls_max;          /* 12    line-search trials */
  int n_refine;        /* 8     most iterative-refinement solves of each Newton system (the Lagrangian
                          Hessian makes the reduced systems stiffer: B2G rnea needs ~6 to
                          reach the sparse LU's direction to 1e-9 with the block inverses); a
                          problem stops refining once a correction is below 1e-12 |dx|_inf or
                          more than 0.9 of the previous one (stagnation); a correction larger
                          than the previous one is not applied and ends the refinement */
  int hessian;         /* PL_IP_HESS_EXACT: the Lagrangian Hessian of f + lam^T g (CasADi's
                          exact Hessian of the Opti/Fatrop solve, ocp.py:248-263) with the
                          inertia correction; PL_IP_HESS_GN: the objective's diagonal only */
} pl_ip_settings;
#define PL_IP_HESS_EXACT 0
#define PL_IP_HESS_GN 1
typedef struct {
  int status, iter, ls_trials, nfilter;
  double err, mu, alpha, alpha_z, f, viol_max;
  double alphas[32];   /* accepted step of each iteration (0: failed line search) */
  int ref_solves;      /* linear solves of the Newton systems of this solve (first solve + the
                          refinement corrections applied), summed over its iterations */
  int pad;
} pl_ip_stats;
int pl_ocp_set_solver(pl_ocp* o, int solver);
int pl_ocp_set_ip_settings(pl_ocp* o, const pl_ip_settings* s);
int pl_ocp_ip_stats(pl_ocp* o, pl_ip_stats* stats);   /* [batch] */
int pl_ocp_get_lam(pl_ocp* o, double* lam);           /* [batch][m]: lam_g (ocp.py:373) */
/* [batch][m] lam_g warm start of the next interior-point solves (the OCPs' warm_start:
 * opti.set_initial(opti.lam_g, lam_g), ocp_whole_body_rnea.py:234-235); NULL = cold
 * (lam = 0, the reference's first solve).  pl_mpc_step carries lam_g itself. */
int pl_ocp_set_lam(pl_ocp* o, const double* lam);
/* Parity aid: the interior point's Newton direction from a given state (x set with
 * pl_ocp_set_x; slacks, multipliers [batch][m], mu [batch]); read it back with
 * pl_debug_get("ip_dx" / "ip_dl" / "ip_ds") and the step bounds with pl_ocp_ip_stats
 * (alpha = primal, alpha_z = bound-multiplier fraction-to-boundary step). */
int pl_debug_ip_direction(pl_ocp* o, const double* s, const double* lam, const double* zl, const double* zu,
                          const double* mu);

/* CasADi external-function ABI (include/pinoloco_casadi.h): bind the OCP whose
 * shapes / sparsity the exported sqp_data, f_data, g_data, hess_data and
 * retract_solution describe (replaces the generated code of ocp.py:299-302 and
 * ocp_whole_body_rnea.py:326-366; retract_steps = num_steps of compile_solution). */
int pl_casadi_bind(pl_ocp* o, int retract_steps);
void pl_casadi_unbind(void);
/* Bind the batch-1 interior-point handle (pl_ocp_set_solver(o, PL_SOLVER_IP)) whose Fatrop
 * solve the exported compiled_solver runs (include/pinoloco_casadi.h; replaces the generated
 * opti.to_function("compiled_solver", ...) of ocp_whole_body_rnea.py:237-258 / ocp.py:324-342,
 * loaded by run_mpc.py:51-53).  warm_start = the compile_solver argument (x_warm_start is then
 * an input); x_initial [n]: the initial guess baked in without it (may be NULL with it).  The
 * parameters the function does not take keep the handle's values at bind time. */
int pl_casadi_bind_compiled(pl_ocp* o, int warm_start, const double* x_initial);
/* Evaluate sqp_data at the current x: any output may be NULL. */
int pl_eval_sqp_data(pl_ocp* o, double* grad, double* Jvals, double* g, double* lbg, double* ubg);
/* f_data value at the current x. */
int pl_eval_f(pl_ocp* o, double* f);
/* Scaled-QP diagnostics after a solve: step dx [batch][n] (unscaled OSQP solution). */
int pl_ocp_get_step(pl_ocp* o, double* dx);

/* Device-side MPC loop (run_mpc.py:127-143) for the whole batch:
 * x_state [batch][nx] = x_init, t0 [batch] = gait time offset. */
int pl_mpc_setup(pl_ocp* o, const double* x_state, const double* t0);
/* One MPC step k: gait schedule at t0 + k*dt_min, x_init, warm start, solve,
 * x_state <- integrate(x_state, DX[1]).  No host transfers.  With the OSQP solver and
 * profiling off, the launches after the gait / warm-start kernel are replayed from a HIP
 * graph captured on the second step with unchanged handle settings (bit-identical to
 * launching them; PL_MPC_GRAPH=0 at creation launches them one by one). */
int pl_mpc_step(pl_ocp* o, int k);
/* The plant of the loop: how the true state x_state moves from step k to k + 1.  The reference
 * closes the loop on the optimiser's own prediction (run_mpc.py:142), which lets no problem
 * deviate from its plan; its commented-out "add noise to x_init" (run_mpc.py:79-82) and its
 * dt_min "used for simulation" (run_mpc.py:18) point at a disturbed, simulated plant.
 * PL_PLANT_ABA, per problem, after the solve of step k:
 *   tau_cmd, f_cmd = tau and forces of node 0 as pl_ocp_retract(steps = 1) returns them (u's tau
 *     block where it exists, else the joint rows of RNEA at the believed state x_init);
 *   (q, v) = x_state, h = dt_min / substeps (the problem's own dt_min parameter);
 *   substeps times: a = ABA(q, v, [w_b; tau_cmd], f_cmd) (pinocchio::aba with f_ext as
 *     dynamics_whole_body_torque.py:55-103 builds it, re-expressed at each substep's q),
 *     q <- integrate(q, v h), v <- v + a h: explicit Euler with the old v, the OCP's own
 *     discretisation (ocp_whole_body_rnea.py:155-158).
 * Without pl_mpc_set_contact (below) there is no contact model: the forces are the commanded
 * ones, world-aligned at the feet and, where the robot has one, the external-force frame.  The
 * setting works on a handle without a device;
 * substeps in [1, 16]; PL_PLANT_ABA needs x = [q, v]: every dynamics kind but centroidal_vel
 * (x = [h, q], dynamics_centroidal_vel.py:12-26).  The OSQP step re-captures its graph once
 * after a change; the interior-point step uses the plant alike. */
#define PL_PLANT_NOMINAL 0   /* x_state <- integrate(x_state, DX[1]) (run_mpc.py:142), the default */
#define PL_PLANT_ABA     1   /* forward dynamics under the commanded torques / forces, above */
int pl_mpc_set_plant(pl_ocp* o, int mode, int substeps);
int pl_mpc_get_plant(const pl_ocp* o, int* mode, int* substeps);
/* Disturbances of the loop, copied into device buffers of the handle; they hold until the next
 * call (a push lasts as many steps as the caller leaves it set) and never re-capture the graph
 * by their values.  base_wrench [batch][6] or NULL (= none): w_b, the generalised force on
 * v[0:6] of the free-flyer, linear then angular, in the base frame (the base rows of
 * pinocchio::aba's tau); read by PL_PLANT_ABA only.  state_noise [batch][ndx] or NULL (= none):
 * the MPC plans from the measured state x_init = state_integrate(x_state, noise)
 * (run_mpc.py:79-82) while x_state stays the true state; under either plant.  Either argument is
 * refused while pl_mpc_set_noise (below) draws that quantity afresh at every step. */
int pl_mpc_set_disturbance(pl_ocp* o, const double* base_wrench, const double* state_noise);
/* Ground contact at the feet and a joint PD loop, options of PL_PLANT_ABA (not a mode of their
 * own).  With them the ground pushes back at the feet instead of the commanded forces, and the
 * joint torque carries a PD term towards node 1 of the plan: the q, v, tau of the first nodes
 * that compile_solution exports for a joint-level PD + feed-forward controller
 * (ocp_whole_body_rnea.py:326-366).  Per problem and substep, for each foot e, in this order:
 *   p = world position of the foot frame, u = its LOCAL_WORLD_ALIGNED linear velocity (at the
 *       substep's q, v);  d = ground_z[e] - p.z
 *   if !(d > 0):  f_e = 0; anchor[e].active = 0                     in the air; lift-off clears the anchor
 *   else  fn = max(0, k_n d - d_n u.z)
 *         if !anchor[e].active: anchor[e].xy = p.xy; active = 1     touchdown
 *         ft = -k_t (p.xy - anchor[e].xy) - d_t u.xy
 *         lim = mu fn;  nrm = sqrt(ft.x^2 + ft.y^2)
 *         if nrm > lim:  ft *= lim / nrm;                           sliding: clamped to the cone,
 *                        if k_t > 0: anchor[e].xy = p.xy + (ft + d_t u.xy) / k_t    the anchor dragged
 *         f_e = (ft.x, ft.y, fn)                                    world-aligned at the foot frame
 *   tau_j = tau_cmd + kp (q_des - q_j) + kd (v_des - v_j)
 *   a = ABA(q, v, [w_b; tau_j], [f_ground(feet) | f_cmd(ext frame)]); q <- integrate(q, v h); v <- v + a h
 * tau_cmd, f_cmd: node 0 of the retract, as above; q_des, v_des: the joint parts of node 1 of the
 * same retract (believed state), held over the step.  The external-force frame keeps its command.
 * Integrator, h and substeps are those of PL_PLANT_ABA.  The ground is flat under each foot at
 * its own height ground_z[batch][n_feet] (steps and holes).  The anchors ([batch][n_feet][3]:
 * x, y, active) are plant state: they persist across substeps and MPC steps, and pl_mpc_setup
 * clears them.  The explicit damping term is the stability limit: h d_n / m_foot < 2 for the
 * lightest foot link; nothing hides it, a plant past it diverges.
 * prm [batch] and ground_z [batch][n_feet]; prm == NULL switches contact and PD off (ground_z
 * ignored).  Refused: k_n <= 0, any negative or non-finite field, centroidal_vel, a handle
 * without a device.  Set while the plant is PL_PLANT_NOMINAL, it is stored and takes effect
 * when PL_PLANT_ABA is selected.  New values and ground heights replay the captured step;
 * switching on or off re-captures once. */
typedef struct { double k_n, d_n, k_t, d_t, mu, kp, kd, pad; } pl_contact_params;   /* one per problem */
int pl_mpc_set_contact(pl_ocp* o, const pl_contact_params* prm, const double* ground_z);
/* any pointer may be NULL: on (0/1), anchors [batch][n_feet][3], the ground forces of the last
 * substep [batch][n_feet][3] */
int pl_mpc_get_contact(pl_ocp* o, int* on, double* anchors, double* forces);
/* One problem's plant step on the host, the same pl::plant_step the kernel runs: p [np], x [n]
 * (the iterate), base_wrench [6] or NULL, prm or NULL (the plain PL_PLANT_ABA step; ground_z and
 * anchors are then not read), anchors [n_feet][3] in/out, x_state [nx] in/out, forces
 * [n_feet][3] out or NULL.  Works on a handle without a device. */
int pl_mpc_plant_host(const pl_ocp* o, const double* p, const double* x, const double* base_wrench,
                      const pl_contact_params* prm, const double* ground_z, double* anchors, int substeps,
                      double* x_state, double* forces);
int pl_mpc_get_state(pl_ocp* o, double* x_state);
/* Solver stats of the last MPC step's (last) SQP iteration, as pl_ocp_solve reports. */
int pl_mpc_get_stats(pl_ocp* o, pl_stats* stats);
/* Copy the first control input row u_0 [batch][nu_0] and x_state into a
 * caller-owned DEVICE buffer (for collectives): layout [batch][nu_0 + nx]. */
int pl_mpc_export(pl_ocp* o, void* device_dst);
/* The same rows [batch][nu_0 + nx] into caller-owned HOST memory, through a pinned staging
 * buffer of the handle; returns after the copy landed (the per-step controller output
 * run_mpc.py:138-141 reads: u_0 and the next state).  bench.py times it beside the step
 * for the PCIe-inclusive rate. */
int pl_mpc_download(pl_ocp* o, double* host_dst);
/* Batched retract of the solved horizon on the device: per problem and node the configuration q,
 * velocity v, acceleration a, contact forces, joint torques tau and eom_base, the base rows of
 * RNEA(q, v, a, forces) (the tau_b whose norm run_mpc.py:232-236 prints).  It is what
 * retract_stacked_sol returns after every solve (optimization/ocp.py:422,
 * ocp_whole_body_rnea.py:293-324, ocp_whole_body_acc.py:195-234, ocp_whole_body_aba.py:177-214,
 * ocp_centroidal_vel.py:195-260), compile_solution exports for the hardware
 * (ocp_whole_body_rnea.py:326-366) and run_mpc.py:186-241 recomputes per node, from the
 * handle's current iterate and each problem's own parameters (x_init, step sizes).  steps in
 * [1, N] nodes from node 0; terminal = 1 (needs steps == N) adds node N's row to q and, where v is
 * part of the state, to v (centroidal_vel: v comes from the inputs, its row count stays steps).
 * Rules the reference's three-node export never reaches: centroidal_vel's node N - 1 reuses the
 * previous node's velocity difference (there is no U[N]); whole_body_rnea nodes without a tau
 * variable (i >= tau_nodes) return the RNEA joint rows (run_mpc.py:211, 233), so tau is always
 * nj wide; whole_body_rnea with include_acc = 0 keeps a 0 columns wide and uses
 * a = (v_{i+1} - v_i) / dt_i inside RNEA (ocp_whole_body_rnea.py:183-191).
 * Valid after pl_ocp_solve and after pl_mpc_step alike: after an MPC step the parameters still
 * hold that step's x_init and the iterate its solution, so there is no pl_mpc_* variant.  A
 * problem that did not converge retracts its current iterate.  pl_mpc_step never launches it.
 *
 * pl_ocp_retract_sizes: out[19] = for each field in the order q, v, a, forces, tau, eom_base
 * its width, row count and offset (doubles) in the packed result, then the total number of
 * doubles of the whole batch.  The packed result is field-major, each field
 * [batch][rows][width].  Works on a handle without a device. */
int pl_ocp_retract_sizes(const pl_ocp* o, int steps, int terminal, long long* out /*[19]*/);
/* The fields into caller-owned HOST arrays [batch][rows][width] (any may be NULL: not copied),
 * through a pinned staging buffer of the handle; returns after the copies landed. */
int pl_ocp_retract(pl_ocp* o, int steps, int terminal, double* q, double* v, double* a, double* forces,
                   double* tau, double* eom_base);
/* The packed result into a caller-owned DEVICE buffer of out[18] doubles; synchronises the
 * handle's stream before returning, as pl_mpc_export does. */
int pl_ocp_retract_device(pl_ocp* o, int steps, int terminal, void* device_dst);
/* MPC-step HIP graph state: out[0] captures, out[1] graph launches, out[2] = 1 when the
 * step fell back to eager launches (a capture or replay failed, or PL_MPC_GRAPH=0). */
int pl_mpc_graph_info(const pl_ocp* o, long long* out);
/* Multipliers across pl_mpc_step with the interior-point solver.  carry = 0 (default): the
 * reference's default driver, solver "fatrop" with compile_solver = True (run_mpc.py:34-37,
 * 50-111): the compiled solver function takes the primal warm start only
 * (ocp_whole_body_rnea.py:239-257), so each solve starts from cold multipliers.  carry = 1: the
 * Opti branch (compile_solver = False, run_mpc.py:115-143 through OCP.solve): warm_start() passes
 * the previous solve's lam_g (ocp_whole_body_rnea.py:234-235, ocp.py:373). */
int pl_mpc_set_ip_lam(pl_ocp* o, int carry);

/* Rollout on the device: a log of what happened at every MPC step, a per-problem outcome, pushes
 * in step windows and a run of steps, with nothing crossing to the host until the caller reads.
 * All of it is off by default, and then pl_mpc_step launches exactly what it launches without it.
 *
 * While the log is on, pl_mpc_step ends with one more launch, outside the captured step (as the
 * gait / warm-start kernel before it), so starting and stopping the log never re-captures.  It
 * writes one row of doubles per problem, fields in this order:
 *   x_init [nx]            the believed state the step planned from (with the state noise)
 *   u0 [nu_0]              the iterate's node-0 inputs, as pl_mpc_download exports them
 *   stats [8]              status, admm_iters, ls_accepted, ls_alpha, viol_max, f, pri_res, dua_res
 *                          of pl_mpc_get_stats for this step
 *   x_state [nx]           the true state after the plant (the state of step k + 1)
 *   ground_f [n_feet * 3]  the ground forces of the last substep (zero while contact is off)
 *   anchor_active [n_feet] 1 where the foot's anchor is set
 * into the log [slot][batch][row].  The s-th step since pl_mpc_log_start (s = 0, 1, ...) is
 * recorded when s % every == 0, into the next of `capacity` slots; with every slot taken it is
 * counted as dropped.  The metrics are updated at every step, recorded or not:
 *   steps            steps seen
 *   first_nonfinite  the first k whose x_state holds a non-finite entry, else -1
 *   first_out        the first k with a finite x_state and |z - z_ref| > dz_tol or c_z < cz_min,
 *                    else -1: z the base height, c_z = 1 - 2 (q_x^2 + q_y^2) of the base quaternion
 *                    (x, y, z, w), the cosine of the base's tilt; z_ref the base height of x_state
 *                    when the log was started (read on the device)
 *   max_dz, min_cz   extrema of |z - z_ref| and c_z over the finite states (start values 0 and 1)
 *   n_not_solved     steps with status != 1;  n_ls_rejected  steps with ls_accepted == 0
 *   max_viol         largest finite viol_max (start value 0) */
typedef struct {
  int steps, first_nonfinite, first_out, n_not_solved, n_ls_rejected, pad;
  double max_dz, min_cz, max_viol;
} pl_mpc_metrics_t;
/* Allocates or reuses the buffers and resets cursor, counters and metrics; after pl_mpc_setup.
 * capacity == 0: metrics only.  dz_tol, cz_min [batch], either may be NULL: never out by that
 * test.  Refused: capacity < 0, every < 1, a non-finite tolerance, a handle without a device;
 * a failed allocation is an error return. */
int pl_mpc_log_start(pl_ocp* o, long long capacity, int every, const double* dz_tol, const double* cz_min);
/* Stops recording (log and metrics); both stay readable. */
int pl_mpc_log_stop(pl_ocp* o);
/* out[17]: width and offset (doubles) inside a row of each field in the order above (out[2 f],
 * out[2 f + 1]), then the row width, capacity, every, recorded, dropped.  The field sizes work
 * on a handle without a device (the last four are then 0). */
int pl_mpc_log_sizes(const pl_ocp* o, long long* out /*[17]*/);
/* Slots [first_slot, first_slot + count) into host_dst [count][batch][row], through the handle's
 * pinned staging buffer; returns after the copy landed.  Refuses slots beyond `recorded`. */
int pl_mpc_log_read(pl_ocp* o, long long first_slot, long long count, double* host_dst);
/* The device address of the log (for collectives; NULL with capacity 0); synchronises the
 * handle's stream, as pl_mpc_export does. */
int pl_mpc_log_device(pl_ocp* o, void** ptr);
int pl_mpc_metrics(pl_ocp* o, pl_mpc_metrics_t* out /*[batch]*/);
/* One problem's record step on the host, the code the device runs: the row of step k from
 * x_init [nx], u0 [nu_0], stats, x_state [nx], ground_f [n_feet][3] (NULL: zeros), anchors
 * [n_feet][3] (x, y, active; NULL: none) and the update of *metrics (the caller's, start values
 * as above on a first step).  dz_tol, cz_min: one value each or NULL.  cursor [5] = {capacity,
 * every, seen, recorded, dropped} of the caller's own log [capacity][row] (NULL with capacity 0):
 * the row is written when the step gets a slot, and seen, recorded, dropped advance.  Works on a
 * handle without a device. */
int pl_mpc_record_host(const pl_ocp* o, int k, const double* x_init, const double* u0, const pl_stats* stats,
                       const double* x_state, const double* ground_f, const double* anchors, double z_ref,
                       const double* dz_tol, const double* cz_min, long long* cursor, double* log,
                       pl_mpc_metrics_t* metrics);
/* Pushes in step windows: while set, step k runs the plant with base wrench wrench[b] when
 * k_start[b] <= k < k_end[b] and zero otherwise (PL_PLANT_ABA reads it, as the base_wrench of
 * pl_mpc_set_disturbance).  k_start, k_end [batch], wrench [batch][6]; all NULL switches the
 * schedule off and zeroes the wrench.  The window is applied by the gait / warm-start kernel,
 * outside the captured step: no re-capture.  While a schedule is set, pl_mpc_set_disturbance
 * with a base_wrench is refused (state noise is unaffected).  Refused before any device work:
 * k_end < k_start, negative steps, non-finite wrench entries. */
int pl_mpc_set_push(pl_ocp* o, const int* k_start, const int* k_end, const double* wrench);
/* Steps k0 ... k0 + steps - 1, exactly a loop of pl_mpc_step: enqueued back to back, with no
 * host synchronisation between them on the OSQP path.  A failing step ends the loop with its
 * error. */
int pl_mpc_run(pl_ocp* o, int k0, int steps);

/* Gait and command timelines: per problem, which gait the loop walks and which targets it tracks
 * at every MPC step, decided on the device (robot.set_gait_sequence and set_tracking_targets
 * between two iterations of run_mpc.py's loop, run_mpc.py:15-24).  Off by default, and then the
 * gait / warm-start launch does exactly what it does without it.
 *
 * A problem's timeline is a list of keyframes sorted by k_start.  At step k the governing
 * keyframe s is the last one with k_start <= k; before the first keyframe the first one governs
 * (clamped).  The gait / warm-start launch of step k then writes into the problem's parameters
 *   1. the commands: base_vel_des always, ext_force_des / arm_vel_des only where the OCP has the
 *      external-force / arm frame.  With ramp == 0, with no keyframe s + 1 or with k < k_start_s
 *      they are keyframe s's, bit for bit; otherwise a = (double)(k - k_s) / (double)(k_{s+1} - k_s)
 *      and c = c_s + a (c_{s+1} - c_s) per component;
 *   2. n_contacts and swing_period of keyframe s's gait: trot 2, period / 2; walk 3, period / 4;
 *      stand 4, period (GaitSequence.__init__, utils/gait_sequence.py:11-21);
 *   3. the contact and swing schedules of the whole horizon for keyframe s's gait and period at
 *      the clock t = (t0[b] + k dt_min) + t_shift_s, the bracket rounded once (a fused
 *      multiply-add, as the device has always computed it).  One gait per solve: it changes between
 *      solves, never inside a horizon;
 *   4. for k > 0 the force warm start, f_des masked by the new schedule, with the new n_contacts.
 * While a timeline is set, a pl_ocp_set_params of the command fields, n_contacts or swing_period
 * is overwritten at the next step.  The keyframes live in device buffers that only that launch
 * reads, outside the captured step: setting, changing or clearing a timeline never re-captures.
 * Both solvers and every plant mode work alike. */
typedef struct {
  int k_start;              /* first MPC step this keyframe governs */
  int gait_type;            /* 0 trot, 1 walk, 2 stand (as pl_ocp_desc.gait_type) */
  int ramp;                 /* 0: hold this keyframe's commands; 1: go linearly to the next keyframe's */
  int pad;
  double gait_period;       /* > 0 */
  double t_shift;           /* added to the gait clock while this keyframe governs (phase alignment at a switch) */
  double base_vel_des[6];
  double ext_force_des[3];  /* ignored where the OCP has no external-force frame */
  double arm_vel_des[3];    /* ignored where it has no arm frame */
} pl_mpc_keyframe;
#define PL_MPC_MAX_KEYFRAMES 64
/* keys [batch][n_key], count [batch] valid keyframes of each problem (NULL: n_key each); entries
 * past a problem's count are never read.  keys == NULL switches the timeline off.  Refused before
 * any device work, with the problem and keyframe in pl_last_error, and leaving a set timeline as
 * it is: n_key outside [1, 64], a count outside [1, n_key], a negative k_start or k_start not
 * strictly increasing within a problem's count, a gait_type outside 0..2, a gait_period that is
 * not finite and positive, a non-finite t_shift or command, a ramp other than 0 or 1, a handle
 * without a device. */
int pl_mpc_set_timeline(pl_ocp* o, int n_key, const pl_mpc_keyframe* keys, const int* count);
int pl_mpc_get_timeline(const pl_ocp* o, int* on, int* n_key);
/* What the last gait / warm-start launch used, per problem: the governing keyframe's index, gait
 * type and period, and the 12 commands it evaluated (base_vel_des, ext_force_des, arm_vel_des;
 * all 12, also those the OCP has no parameter for).  Written by the kernel, read through the
 * pinned staging buffer; any pointer may be NULL.  Needs a timeline. */
int pl_mpc_timeline_state(pl_ocp* o, int* seg /*[batch]*/, int* gait_type /*[batch]*/, double* gait_period /*[batch]*/,
                          double* commands /*[batch][12]*/);
/* One problem's prepare step on the host, the code the kernel runs: steps 1-3 above into p [np]
 * for step k, gait offset t0 and this problem's `count` keyframes, and, for k > 0 with x [n]
 * given, step 4 into x.  *seg (may be NULL): the governing keyframe.  x_init is not touched.
 * Validates the keyframes as pl_mpc_set_timeline does.  Works on a handle without a device. */
int pl_mpc_timeline_host(const pl_ocp* o, int k, double t0, const pl_mpc_keyframe* keys, int count, double* p,
                         double* x, int* seg);

/* Per-step random state noise and base wrench, drawn on the device: the fresh Gaussian draw on
 * x_init at every MPC step that run_mpc.py:79-82 sketches, and per-step process noise on the base
 * wrench.  Off by default, and then the gait / warm-start launch does exactly what it does without
 * it.  The generator is counter-based, Philox4x32-10 (Salmon et al., SC'11): a draw is a pure
 * function of (the problem's seed, the stream, the step k, the component).  It does not depend on
 * the batch size, the problem's slot, the launch geometry, the steps that ran before or the GPU
 * that holds the shard; a rollout restarted at step k continues the same sequence.
 *   block address  counter (k, i, stream, 0), key (seed & 0xffffffff, seed >> 32); i the block
 *                  inside the stream; stream 0 the state noise, 1 the base wrench
 *   uniforms       of the block's words w0..w3, U(a, b) = ((a >> 5) 2^26 + (b >> 6)) 2^-53 (exact, in
 *                  [0, 1)):  u1 = 1 - U(w0, w1),  theta = 0x1.921fb54442d18p+2 U(w2, w3)
 *   normals        r = sqrt(-2 log u1), z_{2i} = r cos theta, z_{2i+1} = r sin theta; component j of
 *                  a stream is normal j & 1 of block j >> 1
 *   state noise    noise_j = state_sigma[b][j] z_j, j < ndx: the MPC of step k plans from
 *                  x_init = state_integrate(x_state, noise) while x_state stays the true state
 *   base wrench    w_c = det_c + wrench_sigma[b][c] z_c, c < 6, product and sum each rounded; det is
 *                  the push window's wrench of step k (pl_mpc_set_push), zero without a schedule;
 *                  read by PL_PLANT_ABA only, as every base wrench
 * The gait / warm-start launch of step k draws them, outside the captured step: switching a stream
 * on or off and new seeds or sigmas never re-capture.  Both solvers and both plants work alike.
 * seed [batch]; state_sigma [batch][ndx] or NULL (that stream off); wrench_sigma [batch][6] or NULL
 * (that stream off).  seed == NULL switches both off and zeroes the base wrench unless a push
 * schedule owns it.  Refused before any device work, with the problem and the component in
 * pl_last_error: a negative or non-finite sigma; seeds without either sigma array.  One owner per
 * buffer: state_sigma is refused while a state_noise of pl_mpc_set_disturbance is set, wrench_sigma
 * while a base_wrench of it is (clear that one first); while a stream is set,
 * pl_mpc_set_disturbance with the matching argument is refused.  A push schedule and the random
 * wrench combine.  Last refusal: a handle without a device.  The settings persist across
 * pl_mpc_setup; there is no generator state to clear. */
int pl_mpc_set_noise(pl_ocp* o, const unsigned long long* seed, const double* state_sigma, const double* wrench_sigma);
int pl_mpc_get_noise(const pl_ocp* o, int* state_on, int* wrench_on);   /* either may be NULL */
/* What the last gait / warm-start launch planned with: the state noise [batch][ndx] and the base
 * wrench [batch][6] in the handle's device buffers (the drawn values while a stream is on, else
 * what pl_mpc_set_disturbance / pl_mpc_set_push left there), read through the pinned staging
 * buffer.  Either pointer may be NULL. */
int pl_mpc_noise_state(pl_ocp* o, double* state_noise, double* base_wrench);
/* One problem's draw of step k >= 0 and its x_init on the host, the code the kernel runs:
 * state_sigma [ndx] or NULL (stream off: zero noise, x_init = x_state), wrench_sigma [6] or NULL
 * (stream off: the wrench is det_wrench), det_wrench [6] or NULL (zero), x_state [nx] (NULL
 * without x_init).  Outputs, each may be NULL: state_noise [ndx], base_wrench [6], x_init [nx].
 * Validates the sigmas as pl_mpc_set_noise does.  Works on a handle without a device. */
int pl_mpc_noise_host(const pl_ocp* o, int k, unsigned long long seed, const double* state_sigma,
                      const double* wrench_sigma, const double* det_wrench, const double* x_state,
                      double* state_noise, double* base_wrench, double* x_init);
/* One Philox4x32-10 block on the host: 32-bit words ctr [4], key [2] -> out [4]. */
int pl_rng_block_host(const unsigned* ctr, const unsigned* key, unsigned* out);
/* The uniforms of one block's words [4] on the host: *u1 = 1 - U(w0, w1) in (0, 1], exact;
 * *theta = 0x1.921fb54442d18p+2 U(w2, w3). */
int pl_rng_uniforms_host(const unsigned* words, double* u1, double* theta);
int pl_ocp_sync(pl_ocp* o);

/* Host-side state maps, x = [q, v], dx = [dq, dv]
 * (DynamicsWholeBodyTorque.state_integrate / state_difference,
 *  dynamics/dynamics_whole_body_torque.py:11-40). */
int pl_state_integrate(const pl_model* m, const double* x, const double* dx, double* out);
int pl_state_difference(const pl_model* m, const double* x0, const double* x1, double* dx);

/* ---- Dynamics plugin surface (dynamics/*.py factories -> batched point functions).
 * A pl_dyn handle holds the contact frames (FR, FL, RR, RL feet, optional
 * external-force frame) and the "base_link" frame of Dynamics.__init__
 * (dynamics/dynamics.py:13-17).  pl_dyn_eval evaluates `batch` points of one
 * function: inputs in0..in3 and the output are caller-owned [batch][len] float64
 * arrays (lengths from pl_dyn_sizes; unused inputs may be NULL).  flags: bit 0 =
 * the forces include the external-force frame (the factories' ext_force_frame
 * argument), bit 1 = relative_to_base (get_frame_velocity).  device >= 0 runs one
 * GPU thread per point; device = -1 evaluates the same code on the host. */
typedef struct pl_dyn pl_dyn;
#define PL_FN_RNEA 0           /* rnea_dynamics(q, v, a, forces) -> tau[nv]      dynamics/dynamics.py:33-65 */
#define PL_FN_ABA 1            /* aba_dynamics(q, v, tau_j, forces) -> a[nv]     dynamics_whole_body_torque.py:73-103 */
#define PL_FN_FRAME_POS 2      /* get_frame_position(frame)(q) -> [3]            dynamics/dynamics.py:67-75 */
#define PL_FN_FRAME_VEL 3      /* get_frame_velocity(frame, rel)(q, v) -> [6]    dynamics/dynamics.py:77-118 */
#define PL_FN_GAPS_WB 4        /* dynamics_gaps(q, v, a, forces) -> [6]          dynamics_whole_body_acc.py:85-126 */
#define PL_FN_BASE_ACC_WB 5    /* base_acc_dynamics(q, v, a_j, forces) -> [6]    dynamics_whole_body_acc.py:43-83 */
#define PL_FN_COM_DYN 6        /* com_dynamics(q, forces) -> h_dot[6]            dynamics_centroidal_vel.py:43-71 */
#define PL_FN_BASE_VEL_CV 7    /* base_vel_dynamics(h, q, v_j) -> v_b[6]         dynamics_centroidal_vel.py:73-89 */
#define PL_FN_BASE_ACC_CV 8    /* base_acc_dynamics(q, v, a_j, forces) -> a_b[6] dynamics_centroidal_vel.py:91-134 */
#define PL_FN_GAPS_CV 9        /* dynamics_gaps(h, q, v) -> A v - m h [6]        dynamics_centroidal_vel.py:136-148 */
#define PL_FN_CRBA 10          /* pinocchio crba(q) -> M[nv][nv]                 run_mpc.py:202 */
#define PL_FN_NLE 11           /* nonLinearEffects(q, v) -> [nv]                 run_mpc.py:203 */
#define PL_FN_FRAME_JAC 12     /* computeFrameJacobian(q, frame, LWA) -> [6][nv] run_mpc.py:206-209 */
#define PL_FN_CMAP 13          /* computeCentroidalMap(q) -> A_G[6][nv]          dynamics_centroidal_vel.py:80 */
#define PL_FN_COM 14           /* centerOfMass(q) -> [3]                         dynamics_centroidal_vel.py:55 */
#define PL_FN_INTEGRATE_WB 15  /* state_integrate (x=[q,v], dx) -> x'            dynamics_whole_body_torque.py:11-25 */
#define PL_FN_DIFFERENCE_WB 16 /* state_difference (x0, x1) -> dx                dynamics_whole_body_torque.py:27-40 */
#define PL_FN_INTEGRATE_CV 17  /* state_integrate (x=[h,q], dx=[dh,dq]) -> x'    dynamics_centroidal_vel.py:12-26 */
#define PL_FN_DIFFERENCE_CV 18 /* state_difference (x0, x1) -> dx                dynamics_centroidal_vel.py:28-41 */
#define PL_FN_GAPS_CA 19       /* dynamics_gaps(q, v, a, forces) -> [6]          dynamics_centroidal_acc.py:92-119 */
int pl_dyn_create(const pl_model* model, const int* foot_frames, int ext_force_frame, int base_frame, int device,
                  pl_dyn** out);
void pl_dyn_destroy(pl_dyn* d);
/* in_len: [4] input lengths, out_len: output length per point. */
int pl_dyn_sizes(const pl_dyn* d, int fn, int flags, int* in_len, int* out_len);
int pl_dyn_eval(pl_dyn* d, int fn, int batch, int frame, int flags, const double* in0, const double* in1,
                const double* in2, const double* in3, double* out);

/* Jacobian of a point function with respect to its inputs, in tangent coordinates (the role of
 * ca.jacobian of the reference's point functions, optimization/ocp.py:283-284).
 *   wrt      bit k selects input k; W = sum of tan_len[k] over the selected inputs; the columns of
 *            jac are the selected inputs' tangents in input order.
 *   jac      caller-owned [batch][out_len][W] float64, row-major per point.
 *   tangent  an input that is a configuration q (length nq: in1 of PL_FN_BASE_VEL_CV and
 *            PL_FN_GAPS_CV, in0 of every other supported function) has tan_len = nv: column k is
 *            d/d eps f(integrate(q, eps e_k)) at eps = 0, integrate = pinocchio's (local free-flyer
 *            twist, linear then angular; revolute coordinates add) -- the convention of
 *            computeRNEADerivatives and of the OCP's own dq columns.  Every other input is
 *            Euclidean: tan_len = in_len.
 *   out      optional [batch][out_len]: the value by the plain double path, bit-identical to
 *            pl_dyn_eval.
 *   supported  PL_FN_RNEA, _ABA, _FRAME_POS, _FRAME_VEL (flags bit 1 as in pl_dyn_eval), _GAPS_WB,
 *            _BASE_ACC_WB, _COM_DYN, _BASE_VEL_CV, _BASE_ACC_CV, _GAPS_CV, _NLE, _COM, _GAPS_CA,
 *            each with flags bit 0 as pl_dyn_eval takes it.
 *   refused  (message in pl_last_error names the function) the matrix-valued PL_FN_CRBA,
 *            _FRAME_JAC, _CMAP; the state maps PL_FN_INTEGRATE_* / _DIFFERENCE_* (their outputs or
 *            branch points live on the manifold, and the OCP rows are linear in dx); wrt == 0; a wrt
 *            bit on an input the function does not take; a missing input; jac == NULL; everything
 *            pl_dyn_eval refuses.  batch == 0 returns 0.
 * pl_dyn_jac_sizes: in_len[4], tan_len[4] (0 for an absent input) and out_len of one point. */
int pl_dyn_jac_sizes(const pl_dyn* d, int fn, int flags, int* in_len, int* tan_len, int* out_len);
int pl_dyn_jac(pl_dyn* d, int fn, int batch, int frame, int flags, unsigned wrt, const double* in0,
               const double* in1, const double* in2, const double* in3, double* out, double* jac);
/* The same with every pointer a DEVICE pointer on the handle's device (refused on a device = -1
 * handle); synchronises the handle's stream before returning, as pl_mpc_export does. */
int pl_dyn_jac_device(pl_dyn* d, int fn, int batch, int frame, int flags, unsigned wrt, const void* in0,
                      const void* in1, const void* in2, const void* in3, void* out, void* jac);

/* ADMM linear-solve kernel.  All of them run the same OSQP 0.6 iteration on the same
 * block factor and agree to round-off; they differ in how the block-tridiagonal solve is
 * mapped to the GPU.  PL_ADMM_AUTO picks by batch size;
 * PL_ADMM_SWEEP: one wave per problem, node-by-node sweeps (large batches);
 * PL_ADMM_SWEEP2: two waves per problem; PL_ADMM_CHAIN: reduced chain, one workgroup
 * per problem (small batches).  Internal to osqp.solve() (optimization/ocp.py:401). */
#define PL_ADMM_AUTO 0
#define PL_ADMM_SWEEP 1
#define PL_ADMM_SWEEP2 2
#define PL_ADMM_CHAIN 3
int pl_ocp_set_admm_kernel(pl_ocp* o, int kind);
int pl_ocp_get_admm_kernel(const pl_ocp* o);
/* Workgroups per problem of the next ADMM launch: 1 for the sweep kernels; for the chain kernel
 * ceil((N + 1) / 8) while the batch's workgroups fit one per CU, else fewer (1 under
 * PL_PATH_RC_ONE_GROUP). */
int pl_ocp_get_admm_groups(const pl_ocp* o);
/* Small operands of the PL_ADMM_SWEEP kernel.  PL_ADMM_OPERANDS_FUSED (default): a step issues
 * only the loads it consumes, and rho comes from the row bounds the step already holds where
 * the OSQP path wrote it by its rule.  PL_ADMM_OPERANDS_SPLIT: the earlier path (every array on its own, every prefetch issued),
 * kept as the regression reference.  Results are bit-identical; the other kernels ignore it.
 * pl_ocp_get_admm_rho_from_bounds: 1 when a fused sweep launched now would compute rho from
 * the bounds, 0 when it would stream it (after an interior-point solve, or in SPLIT mode). */
#define PL_ADMM_OPERANDS_SPLIT 0
#define PL_ADMM_OPERANDS_FUSED 1
int pl_ocp_set_admm_operands(pl_ocp* o, int mode);
int pl_ocp_get_admm_operands(const pl_ocp* o);
int pl_ocp_get_admm_rho_from_bounds(const pl_ocp* o);

/* OSQP's adaptive_rho (OSQP 0.6.x compute_rho_estimate / adapt_rho / osqp_update_rho; the
 * reference switches it off, optimization/ocp.py:267-273, and so does the default here).  Every
 * problem of the batch holds its own rho, initialised to the handle's rho by pl_ocp_init_solver
 * and by every call of the setter, and carried from one solve to the next (SQP iterations, MPC
 * steps, warm-started solves) as OSQP carries settings->rho.  At every termination check whose
 * iteration is a multiple of `interval`, a problem that the exact pass did not terminate
 * estimates, on the solver's scaled quantities (infinity norms),
 *   rho_est = clip(rho sqrt((|Ax - z| / (max(|z|, |Ax|) + 1e-10)) /
 *                           (|Px + q + A'y| / (max(|q|, |A'y|, |Px|) + 1e-10) + 1e-10)), 1e-6, 1e6)
 * and, iff rho_est > rho * tolerance or rho_est < rho / tolerance, takes it: the problem's row
 * weights are rewritten by OSQP's classes, the problem is refactored and its right-hand side is
 * rebuilt; the iterates are not touched.  At iteration max_iter the new rho serves the next solve.
 * interval: 0 = check_termination, else a positive multiple of it (OSQP's automatic interval is a
 * fraction of the measured setup time, not deterministic, and is not offered); tolerance > 1
 * (OSQP: 5).  The setter fails with a message otherwise.  While the option is on, the fused sweep
 * streams rho (pl_ocp_get_admm_rho_from_bounds is 0).  With PL_SOLVER_IP the settings are stored
 * and have no effect.  pl_ocp_get_rho: per problem, rho, the last estimate and the number of
 * updates in the last solve (any of the three may be null).
 * pl_osqp_rho_estimate_host: the rule itself on the host, the code the kernel runs; norms =
 * |Ax - z|, |z|, |Ax|, |Px + q + A'y|, |q|, |A'y|, |Px|. */
int pl_ocp_set_adaptive_rho(pl_ocp* o, int enable, int interval, double tolerance);
int pl_ocp_get_adaptive_rho(const pl_ocp* o, int* enable, int* interval, double* tolerance);
int pl_ocp_get_rho(pl_ocp* o, double* rho, double* rho_estimate, int* updates);
int pl_osqp_rho_estimate_host(const double norms[7], double rho, double tol, double* rho_est, int* update);

/* Timing of the dominant kernel (ADMM sweeps) with HIP events on the handle's
 * stream: pl_ocp_profile(o, 1) clears and starts, pl_ocp_profile_read returns
 * [total_ms, launches, problem_iterations]. pl_ocp_sizes (out[13]): [n, m, nnz,
 * factor doubles per problem, largest node block, N, ADMM gather program length
 * (u16 words, LDS-resident), problems per ADMM workgroup, ADMM LDS bytes per
 * workgroup, A values per thread, A values per problem staged in LDS by the sweep,
 * largest node's A count, the descriptor's debug_paths bits]. */
int pl_ocp_profile(pl_ocp* o, int enable);
int pl_ocp_profile_read(pl_ocp* o, double* out);
/* The same for the interior point's Lagrangian-Hessian launches (k_lag_hess_*): out[0] total ms,
 * out[1] launches, out[2] problem lanes per launch (the active problems rounded up to whole
 * waves; bench.py --solver fatrop scales the per-launch flops by it). */
int pl_ocp_profile_read_hess(pl_ocp* o, double* out);
int pl_ocp_sizes(const pl_ocp* o, long long* out);

/* Test / parity access to internal per-problem arrays and the node table. */
int pl_debug_get(pl_ocp* o, const char* name, double* out, long long count);
int pl_debug_set(pl_ocp* o, const char* name, const double* in, long long count);
int pl_debug_nodes(const pl_ocp* o, int* out);
int pl_debug_consts(const pl_ocp* o, void* model_out, void* oc_out, int* sizes);
/* reset bit 0: start from x = z = y = 0; bit 1: the last iteration stores delta x / delta y
 * ("dxs", "dys") as a check iteration of pl_ocp_solve does. */
int pl_debug_admm(pl_ocp* o, int niter, int reset);
/* Ruiz scaling + scaled data alone on the raw arrays as they are (no evaluation, no factor). */
int pl_debug_qp_setup(pl_ocp* o);
/* The gait / warm-start launch of MPC step k alone (random draw, x_init, push window, timeline,
 * schedule, warm start), then a synchronise: p and x can be read before any solve overwrites the iterate. */
int pl_debug_mpc_prepare(pl_ocp* o, int k);
/* The device's raw Philox blocks for the seeds given to pl_mpc_set_noise: block i < n_blocks of
 * problem b has the counter (k, i0 + i, stream, c3) and the key of seed[b]; the loop's draws have
 * i0 = c3 = 0.  out [batch][n_blocks][4] 32-bit words.  The integer part of the generator, to be
 * compared bit for bit away from any libm. */
int pl_debug_rng(pl_ocp* o, unsigned k, unsigned stream, unsigned i0, unsigned c3, int n_blocks, unsigned* out);
/* One termination check on the current iterates and scaled data, then (unscale) the step
 * write-back; read status / pri_res / dua_res with pl_mpc_get_stats. */
int pl_debug_check(pl_ocp* o, int final_check, int unscale);
/* Interior-point stage tests: exactly one stage of the interior-point iteration on the device
 * buffers as they are (pl_ocp_set_solver(o, PL_SOLVER_IP) first), then a synchronise.
 *   PL_IP_STAGE_INIT     k_ip_init with warm = arg, on the current "g", "lbg", "ubg" (and
 *                        "ip_lam0"); nothing is evaluated first
 *   PL_IP_STAGE_KKT      k_ip_kkt of iteration k = arg >= 0 on the current "g", "lbg", "ubg",
 *                        "Araw", "grad", "P", "work"[0], slacks and multipliers; nothing is
 *                        evaluated first
 *   PL_IP_STAGE_INERTIA  one launch of k_ip_inertia (cap 8) on the current "ip_iflag", "ip_dwi",
 *                        "P", "Ps"
 *   PL_IP_STAGE_STEP     the rows and the objective at the current x, then k_ip_step with the
 *                        line search and the update, on the current "ip_dx", "ip_jdx", "xa", "za",
 *                        "rho", "ip_rh", slacks, multipliers and "ipinfo"
 * pl_debug_get / pl_debug_set names that serve them: "work" ([batch][8], [0] = f), "ip_iflag"
 * ([batch][4] ints as doubles), "info_done" ([batch], PlProbInfo::done as a double) and "ipinfo",
 * [batch][PL_IPINFO_DOUBLES] with the fields in this order (ints as doubles):
 *   0 mu, 1 theta_max, 2 theta_min, 3 err, 4 f, 5 alpha, 6 alpha_z, 7 viol_max, 8 iter,
 *   9 status, 10 nfilt, 11 trials, 12 active, 13 ref_solves, 14 ref_last,
 *   15 .. 78 filt[64] ((theta, phi) pairs), 79 .. 110 alphas[32] */
#define PL_IP_STAGE_INIT 0
#define PL_IP_STAGE_KKT 1
#define PL_IP_STAGE_INERTIA 2
#define PL_IP_STAGE_STEP 3
#define PL_IPINFO_DOUBLES 111
int pl_debug_ip_stage(pl_ocp* o, int stage, int arg);

#ifdef __cplusplus
}
#endif
#endif /* PINOLOCO_H_ */
