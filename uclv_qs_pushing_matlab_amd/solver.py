"""Batched acados-style OCP solver object over the HIP C ABI.

`OcpSolver` stands where the reference creates `acados_ocp(ocp_model, ocp_opts)`
(acados_nmpc/NMPC_controller.m:302-305) and drives it with `.set/.solve/.get`
(:154-157, 170, 334-348, 382-394, 403, 420; helper.m:253, 264-269).  Every per-lane
quantity carries a leading batch dimension B; one call solves B OCPs on the GPU.
Field names and stage semantics follow the acados MATLAB interface; unknown fields
raise KeyError, wrong shapes raise ValueError (the reference's MEX raises MATLAB
errors in both cases); numerical failure is reported per lane through 'status'.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64, i32, ptr


class OcpSolver:
    # nlp_solver_type (NMPC_controller.m:271): 'SQP_RTI' = fixed-K full steps (the BASELINE
    # metric), 'SQP' = merit backtracking + KKT tolerances (the reference's own options)
    NLP_MODES = {"SQP_RTI": 0, "SQP": 1}

    def __init__(self, N=20, batch=1, Ts=0.05, sqp_iters=50, qp_iters=20, stages_per_lane=0, device=0,
                 cost_scale_Ts=True, mu0=1.0, t_min=1e-2, frac=0.995, sigma_min=1e-2, mu_stop=1e-10, res_stop=1e-10,
                 qp_tol_stat=1e-10, qp_tol_eq=1e-10, stage0_s_bound=True, qp_stall_iters=3, qp_stall_alpha=1e-3,
                 qp_mu_max=1e100, factor_scan=False,
                 nlp_solver_type="SQP_RTI", tol=1e-6, ls_alpha_min=0.05, ls_alpha_red=0.7, ls_eps=1e-4,
                 qp_solver_cond_N=None, timings=False):
        # qp_solver_cond_N (NMPC_controller.m:276) selects HPIPM's partial condensing, a different
        # factorisation of the same QP.  The kernel factorises stage-wise at every value: condensed
        # blocks measured 1.16-3.1x slower (profiles/r03/cond_block.txt).  The
        # value is checked (1..N) and kept as .qp_solver_cond_N.
        if qp_solver_cond_N is not None and (int(qp_solver_cond_N) != qp_solver_cond_N
                                             or not 1 <= qp_solver_cond_N <= N):
            raise ValueError("qp_solver_cond_N must be an integer in 1..N")
        self.qp_solver_cond_N = int(N if qp_solver_cond_N is None else qp_solver_cond_N)
        L = _lib.lib()
        o = _lib.Options()
        L.qsp_default_options(C.byref(o))
        o.N, o.batch, o.Ts = int(N), int(batch), float(Ts)
        o.sqp_iters, o.qp_iters, o.stages_per_lane, o.device = int(sqp_iters), int(qp_iters), int(stages_per_lane), int(device)
        o.cost_scale_Ts = 1 if cost_scale_Ts else 0
        o.mu0, o.t_min, o.frac, o.sigma_min, o.mu_stop = mu0, t_min, frac, sigma_min, mu_stop
        o.res_stop = res_stop
        o.qp_tol_stat, o.qp_tol_eq = float(qp_tol_stat), float(qp_tol_eq)
        o.stage0_s_bound = 1 if stage0_s_bound else 0
        o.qp_stall_iters, o.qp_stall_alpha = int(qp_stall_iters), float(qp_stall_alpha)
        o.qp_mu_max = float(qp_mu_max)
        # two stages per lane (N + 1 > 32): the factorisation as an associative scan (faster, less
        # accurate; include/qsp_nmpc.h)
        o.factor_scan = 1 if factor_scan else 0
        if nlp_solver_type not in self.NLP_MODES:
            raise ValueError(f"nlp_solver_type must be one of {tuple(self.NLP_MODES)}")
        o.nlp_mode = self.NLP_MODES[nlp_solver_type]
        o.tol_stat = o.tol_eq = o.tol_ineq = o.tol_comp = float(tol)
        o.ls_alpha_min, o.ls_alpha_red, o.ls_eps = float(ls_alpha_min), float(ls_alpha_red), float(ls_eps)
        h = C.c_void_p()
        check(L.qsp_create(C.byref(o), C.byref(h)), "qsp_create")
        self._L, self._h, self.opts = L, h, o
        self.N, self.B, self.Ts = o.N, o.batch, o.Ts
        Bn, Nn = self.B, self.N
        self._x0 = np.zeros((Bn, 4))
        self._yref = np.zeros((Bn, Nn, 6))
        self._yref_e = np.zeros((Bn, 4))
        self._X = np.zeros((Bn, Nn + 1, 4))
        self._U = np.zeros((Bn, Nn, 2))
        self._PI = np.zeros((Bn, Nn, 4))
        self._W = np.array([1.0, 1.0, 1e-3, 0.0, 1e-3, 1e-3])
        self._We = np.array([2e5, 2e5, 20.0, 0.0])
        self._lh = np.array([-0.06, 0.0, -0.05])
        self._uh = np.array([0.011, 0.03, 0.05])
        self._dirty = set(["x0", "yref", "init"])
        self._refs_staged = False   # the device references are a controller step's, newer than set('cost_y_ref*')
        self._refs_given = False    # set('cost_y_ref*') was called: eval_kkt may flush them (else the zeros above are no reference)
        self.n_shapes = 0
        self.shape_ids = np.zeros(Bn, np.int32)   # host copy of the per-lane shape ids (helper.mode_trace)
        self._plant = None                        # host copy of the installed plant model (set_plant)
        self._noise_scale = None                  # host copy of the installed generator's lane_scale (set_sim_noise)
        # timings=True: per-kernel HIP events around every solve, for get('time_lin'/'time_qp_sol')
        self._timings = bool(timings)
        self._last_times = None

    # ------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self._L.qsp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def layout(self):
        S, L = C.c_int32(), C.c_int32()
        check(self._L.qsp_get_layout(self._h, C.byref(S), C.byref(L)), "qsp_get_layout")
        return S.value, L.value

    FACTOR_WALKS = {0: "lane walk", 1: "matrix cores (v_mfma_f64_4x4x4_4b_f64)", 2: "associative scan"}

    def factor_walk(self):
        """How the QPs walk the horizon, as the library reports it (qsp_get_factor_walk, QSP_WALK_*)."""
        w = C.c_int32()
        check(self._L.qsp_get_factor_walk(self._h, C.byref(w)), "qsp_get_factor_walk")
        return self.FACTOR_WALKS[w.value]

    def fixed_horizon(self):
        """The horizon the per-iteration QP launches are compiled for (qsp_get_fixed_horizon; 0: none)."""
        n = C.c_int32()
        check(self._L.qsp_get_fixed_horizon(self._h, C.byref(n)), "qsp_get_fixed_horizon")
        return n.value

    # --------------------------------------------------------------- model
    def set_shapes(self, shapes, shape_id=None):
        arr = (_lib.Shape * len(shapes))(*shapes)
        check(self._L.qsp_set_shapes(self._h, arr, len(shapes)), "qsp_set_shapes")
        self.n_shapes = len(shapes)
        if shape_id is not None:
            self.set_shape_ids(shape_id)

    def set_shape_ids(self, shape_id):
        sid = i32(np.broadcast_to(np.asarray(shape_id, np.int32), (self.B,)))
        check(self._L.qsp_set_shape_ids(self._h, ptr(sid)), "qsp_set_shape_ids")
        self.shape_ids = sid.copy()

    # ------------------------------------------- the plant's own model
    def _install_plant(self, p):
        """The handle's plant <- p (a plant() dict or None), from a cleared state."""
        check(self._L.qsp_clear_plant(self._h), "qsp_clear_plant")
        self._plant = None
        if p is None:
            return
        if p["shapes"] is not None:
            arr = (_lib.Shape * len(p["shapes"]))(*p["shapes"])
            check(self._L.qsp_set_plant_shapes(self._h, arr, len(p["shapes"])), "qsp_set_plant_shapes")
            if p["shape_id"] is not None:
                check(self._L.qsp_set_plant_shape_ids(self._h, ptr(p["shape_id"])), "qsp_set_plant_shape_ids")
        if p["mu_sp"] is not None or p["c_ellipse"] is not None:
            check(self._L.qsp_set_plant_params(self._h, ptr(p["mu_sp"]), ptr(p["c_ellipse"])), "qsp_set_plant_params")
        self._plant = p

    def set_plant(self, shapes=None, shape_id=None, mu_sp=None, c_ellipse=None):
        """The model that closed_loop simulates with, where it is not the controller's (closed_loop_matlab's
        `plant` argument, helper.m:195-322): the plant step, the delay prediction, the disturbance
        re-projection and the mode counts of closed_loop_metrics read it; the solve keeps the controller's.
        shapes: a plant shape table with shape_id (scalar or (B,), default 0) into it; None: the controller's
        shapes.  mu_sp, c_ellipse: scalar or (B,) overrides of the plant shape's two constants, finite and
        > 0.  Replaces what was installed; all None is clear_plant().  When the library rejects an argument
        the plant installed before the call is put back."""
        if shapes is None and shape_id is not None:
            raise ValueError("set_plant: shape_id needs a plant shape table (shapes)")
        lanes = lambda v: None if v is None else f64(np.broadcast_to(np.asarray(v, np.float64), (self.B,)))  # noqa: E731
        p = dict(shapes=None if shapes is None else list(shapes),
                 shape_id=None if shape_id is None else i32(np.broadcast_to(np.asarray(shape_id, np.int32), (self.B,))),
                 mu_sp=lanes(mu_sp), c_ellipse=lanes(c_ellipse))
        if all(v is None for v in p.values()):
            p = None
        prev = self._plant
        try:
            self._install_plant(p)
        except Exception:
            self._install_plant(prev)
            raise

    def clear_plant(self):
        """Back to "the plant is the controller's model", the state of a new solver."""
        self._install_plant(None)

    def plant(self):
        """What set_plant installed: None, or dict(shapes, shape_id, mu_sp, c_ellipse) with None for what
        is left to the controller's model / the plant shape.  set_plant(**p) installs such a dict again."""
        hs, hp = C.c_int32(), C.c_int32()
        check(self._L.qsp_get_plant(self._h, C.byref(hs), C.byref(hp)), "qsp_get_plant")
        p = self._plant
        want = (0, 0) if p is None else (0 if p["shapes"] is None else len(p["shapes"]),
                                         (p["mu_sp"] is not None) | 2 * (p["c_ellipse"] is not None))
        if (hs.value, hp.value) != want:
            raise _lib.QspError(f"plant(): the handle reports {(hs.value, hp.value)}, this object installed {want}")
        return None if p is None else dict(p)

    # ------------------------------------ sim_noise generated on the device
    def set_sim_noise(self, seed, sigma=None, lane_scale=None, stream=0, step_offset=0, lane_offset=0):
        """Install the sim_noise generator (qsp_set_sim_noise; helper.m:240-242, :154-156): with it and
        noise=None, closed_loop, closed_loop_metrics, open_loop and open_loop_device draw x += (sigma *
        lane_scale[lane]) * randn(4) in their kernels, a pure function of (seed, stream, lane_offset + lane,
        step_offset + step): no table, and shards (lane_offset) and chunks (step_offset) of a run draw the whole
        run's numbers.  sigma (4,), None: the reference's 1e-5, 1e-5, 1e-3, 1e-4; lane_scale scalar or (B,),
        None: 1.  Replaces what was installed; an argument the library rejects leaves it."""
        g = _lib.SimNoise()
        self._L.qsp_default_sim_noise(C.byref(g))
        g.seed, g.stream = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF
        g.step_offset, g.lane_offset = int(step_offset), int(lane_offset)
        if sigma is not None:
            g.sigma[:] = [float(v) for v in np.asarray(sigma, np.float64).reshape(4)]
        sc = None if lane_scale is None else f64(np.broadcast_to(np.asarray(lane_scale, np.float64), (self.B,)))
        g.lane_scale = None if sc is None else sc.ctypes.data
        check(self._L.qsp_set_sim_noise(self._h, C.byref(g)), "qsp_set_sim_noise")
        self._noise_scale = None if sc is None else sc.copy()

    def clear_sim_noise(self):
        """No generator: noise comes from a table or not at all, the state of a new solver."""
        check(self._L.qsp_clear_sim_noise(self._h), "qsp_clear_sim_noise")
        self._noise_scale = None

    def get_sim_noise(self):
        """What set_sim_noise installed, as the handle reports it: None, or dict(seed, sigma, lane_scale, stream,
        step_offset, lane_offset); set_sim_noise(**d) installs such a dict again."""
        g, on, sc = _lib.SimNoise(), C.c_int32(), C.c_int32()
        check(self._L.qsp_get_sim_noise(self._h, C.byref(g), C.byref(on), C.byref(sc)), "qsp_get_sim_noise")
        if not on.value:
            return None
        return dict(seed=g.seed, sigma=np.array(g.sigma[:]), lane_scale=self._noise_scale.copy() if sc.value else None,
                    stream=g.stream, step_offset=g.step_offset, lane_offset=g.lane_offset)

    def gen_sim_noise(self, n_steps):
        """The table the loops draw over n_steps steps with the installed generator: (n_steps, B, 4)."""
        out = np.zeros((int(n_steps), self.B, 4))
        check(self._L.qsp_gen_sim_noise(self._h, int(n_steps), ptr(out)), "qsp_gen_sim_noise")
        return out

    # ----------------------------------------------------------------- set
    def _lanes(self, v, width):
        v = np.asarray(v, np.float64)
        if v.shape == (width,) or v.shape == (width, 1):
            return np.broadcast_to(v.reshape(width), (self.B, width))
        if v.shape == (self.B, width):
            return v
        raise ValueError(f"expected ({width},) or ({self.B},{width}), got {v.shape}")

    def set(self, field, value, stage=None):
        N = self.N
        if field == "constr_x0":
            self._x0[:] = self._lanes(value, 4)
            self._dirty.add("x0")
        elif field == "cost_y_ref":
            if stage is None:
                v = np.asarray(value, np.float64)
                if v.shape not in ((self.B, N, 6), (N, 6)):
                    raise ValueError(f"cost_y_ref without stage expects (B,N,6) or (N,6), got {v.shape}")
                self._yref[:] = v
            else:
                if not 0 <= stage < N:
                    raise ValueError(f"cost_y_ref stage {stage} out of range 0..{N - 1}")
                self._yref[:, stage] = self._lanes(value, 6)
            self._dirty.add("yref")
            self._refs_staged = False
            self._refs_given = True
        elif field == "cost_y_ref_e":
            if stage is not None and stage != N:
                raise ValueError("cost_y_ref_e is only defined at stage N")
            self._yref_e[:] = self._lanes(value, 4)
            self._dirty.add("yref")
            self._refs_staged = False
            self._refs_given = True
        elif field == "cost_W":
            W = np.asarray(value, np.float64)
            if W.ndim == 2:
                if np.any(W != np.diag(np.diag(W))):
                    raise ValueError("cost_W: only diagonal weights are supported")
                W = np.diag(W)
            if stage == N:
                if W.shape != (4,):
                    raise ValueError("cost_W at stage N must be 4x4")
                self._We[:] = W
            else:
                if W.shape != (6,):
                    raise ValueError("cost_W must be 6x6")
                self._W[:] = W
            check(self._L.qsp_set_cost_W(self._h, ptr(f64(self._W)), ptr(f64(self._We))), "qsp_set_cost_W")
        elif field in ("constr_lh", "constr_uh"):
            v = np.asarray(value, np.float64).reshape(3)
            (self._lh if field == "constr_lh" else self._uh)[:] = v
            check(self._L.qsp_set_constr_h(self._h, ptr(f64(self._lh)), ptr(f64(self._uh))), "qsp_set_constr_h")
        elif field == "init_x":
            v = np.asarray(value, np.float64)
            self._X[:] = v.reshape(self._X.shape) if v.size == self._X.size else np.broadcast_to(v, self._X.shape)
            self._dirty.add("init")
        elif field == "init_u":
            v = np.asarray(value, np.float64)
            self._U[:] = v.reshape(self._U.shape) if v.size == self._U.size else np.broadcast_to(v, self._U.shape)
            self._dirty.add("init")
        elif field == "init_pi":
            v = np.asarray(value, np.float64)
            self._PI[:] = v.reshape(self._PI.shape) if v.size == self._PI.size else np.broadcast_to(v, self._PI.shape)
            self._dirty.add("init")
        else:
            raise KeyError(f"OcpSolver.set: unknown field '{field}'")

    def set_ctrl_params(self, v_alpha, d_v_bound, t_angle0, u_n_lb, u_t_ub):
        check(self._L.qsp_set_ctrl_params(self._h, v_alpha, d_v_bound, t_angle0, u_n_lb, u_t_ub), "qsp_set_ctrl_params")

    # --------------------------------------------------------------- solve
    def _flush(self):
        if "x0" in self._dirty:
            check(self._L.qsp_set_x0(self._h, ptr(f64(self._x0))), "qsp_set_x0")
        if "yref" in self._dirty:
            check(self._L.qsp_set_yref(self._h, ptr(f64(self._yref)), ptr(f64(self._yref_e))), "qsp_set_yref")
            self._refs_staged = False
        if "init" in self._dirty:
            check(self._L.qsp_set_init(self._h, ptr(f64(self._X)), ptr(f64(self._U)), ptr(f64(self._PI))),
                  "qsp_set_init")
        self._dirty.clear()

    def _timed(self, fn, *args):
        if self._timings:
            self.set_kernel_timing(1)
        fn(*args)
        if self._timings:
            self._last_times = self.kernel_times()

    def solve(self):
        self._flush()
        self._timed(lambda: check(self._L.qsp_solve(self._h), "qsp_solve"))

    # ----------------------------------------------------------------- get
    def get(self, field, stage=None):
        B, N = self.B, self.N
        if field in ("x", "u", "pi"):
            shape = {"x": (B, N + 1, 4), "u": (B, N, 2), "pi": (B, N, 4)}[field]
            out = np.zeros(shape)
            fn = {"x": self._L.qsp_get_x, "u": self._L.qsp_get_u, "pi": self._L.qsp_get_pi}[field]
            check(fn(self._h, ptr(out)), f"get('{field}')")
            return out if stage is None else out[:, stage]
        if field in ("status", "sqp_iter", "qp_iter", "qp_capped", "qp_stalled"):
            out = np.zeros(B, np.int32)
            fn = {"status": self._L.qsp_get_status, "sqp_iter": self._L.qsp_get_sqp_iter,
                  "qp_iter": self._L.qsp_get_qp_iter, "qp_capped": self._L.qsp_get_qp_capped,
                  "qp_stalled": self._L.qsp_get_qp_stalled}[field]
            check(fn(self._h, ptr(out)), f"get('{field}')")
            return out
        if field == "modes":       # contact mode of stage k at (x_k, u_k) of get('x') / get('u'), k = 0..N-1
            out = self.get_modes()
            return out if stage is None else out[:, stage]
        if field == "residuals":   # acados res_stat/eq/ineq/comp of the last KKT test (nlp_mode 1)
            out = np.zeros((B, 4))
            check(self._L.qsp_get_residuals(self._h, ptr(out)), "get('residuals')")
            return out
        if field == "lam":         # acados get('lam'): bound multipliers of the final NLP iterate (nlp_mode 1), never shifted
            out = np.zeros((B, N, 6))
            check(self._L.qsp_get_lam(self._h, ptr(out)), "get('lam')")
            return out if stage is None else out[:, stage]
        if field == "sens_K0":     # the feedback gain du_0/dx0 at the last solve()'s iterate (get_sens)
            return self.get_sens()["K0"]
        if field == "time_tot":
            ms = C.c_double()
            check(self._L.qsp_get_time_tot(self._h, C.byref(ms)), "get('time_tot')")
            return ms.value * 1e-3
        if field in ("time_lin", "time_qp_sol"):                # helper.m:264-269, seconds
            if self._last_times is None:
                raise KeyError(f"get('{field}') needs OcpSolver(..., timings=True) and a solve")
            key = "linearize" if field == "time_lin" else "qp_step"
            return self._last_times[key][0] * 1e-3
        raise KeyError(f"OcpSolver.get: unknown field '{field}'")

    def get_u0(self):
        out = np.zeros((self.B, 2))
        check(self._L.qsp_get_u0(self._h, ptr(out)), "qsp_get_u0")
        return out

    def get_cost(self):
        out = np.zeros(self.B)
        check(self._L.qsp_get_cost(self._h, ptr(out)), "qsp_get_cost")
        return out

    # ------------------------------- KKT residuals recomputed on the device
    def eval_kkt(self, x=None, u=None, pi=None, lam=None, x0=None, yref=None, yref_e=None, parts=False, stages=False):
        """KKT residuals of an NLP iterate recomputed from its numbers (qsp_eval_kkt): res (B, 4) in acados'
        order res_stat, res_eq, res_ineq, res_comp; with parts / stages a tuple (res[, parts (B, 7), columns
        _lib.KKT_PARTS][, stage_res (B, N + 1, 4)]).  Works in both nlp_solver_types and needs no solve.
        x, u, pi omitted: get('x'), get('u'), get('pi').  lam omitted: get('lam') with 'SQP', and the implied
        multipliers with 'SQP_RTI', which keeps none (lam='implied' asks for them with 'SQP' too): each
        bounded quantity takes lam_lo = max(r, 0), lam_hi = max(-r, 0) from its stationarity r, and the
        optimality gap shows in res_comp.  x0 None: x's row 0 is the initial state; else used as given,
        without the controller's s pre-wrap.  yref / yref_e None: the handle's references.
        The defaults are meaningful after solve(), not after controller_solve(): its get('x'), get('u') and
        get('pi') are the warm start shifted by one stage, while get('lam') and the staged references are
        the unshifted step's."""
        B, N = self.B, self.N
        X = f64(self.get("x") if x is None else x, (B, N + 1, 4))
        U = f64(self.get("u") if u is None else u, (B, N, 2))
        PI = f64(self.get("pi") if pi is None else pi, (B, N, 4))
        if lam is None:
            lam = self.get("lam") if self.opts.nlp_mode == self.NLP_MODES["SQP"] else "implied"
        LAM = None if isinstance(lam, str) and lam == "implied" else f64(lam, (B, N, 6))
        x0 = None if x0 is None else f64(self._lanes(x0, 4))
        yr, ye = self._rollout_refs(yref, yref_e, flush=self._refs_given)
        res = np.zeros((B, 4))
        pt = np.zeros((B, len(_lib.KKT_PARTS))) if parts else None
        sr = np.zeros((B, N + 1, 4)) if stages else None
        check(self._L.qsp_eval_kkt(self._h, ptr(x0), ptr(X), ptr(U), ptr(PI), ptr(LAM), ptr(yr), ptr(ye), ptr(res),
                                   ptr(pt), ptr(sr)), "qsp_eval_kkt")
        out = (res,) + ((pt,) if parts else ()) + ((sr,) if stages else ())
        return out[0] if len(out) == 1 else out

    def eval_kkt_device(self, io, stream=None):
        """eval_kkt on caller-owned device memory (io: _lib.KktIO of device pointers), asynchronous."""
        check(self._L.qsp_eval_kkt_device(self._h, C.byref(io), C.c_void_p(stream) if stream else None),
              "qsp_eval_kkt_device")

    # ------------------------------- solution sensitivities du_k/dx0
    @staticmethod
    def _sens_want(want):
        """The outputs asked for, checked before any library call: names of _lib.SENS_OUTPUTS."""
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in _lib.SENS_OUTPUTS]
        if bad:
            raise ValueError(f"want: unknown output(s) {bad}; choose from {_lib.SENS_OUTPUTS}")
        return want

    def _sens_opts(self, t_floor, s0_bound):
        o = _lib.SensOpts()
        self._L.qsp_default_sens_opts(C.byref(o))
        o.t_floor = float(t_floor)
        o.s0_bound = -1 if s0_bound is None else int(bool(s0_bound))
        return o

    @staticmethod
    def _sens_outputs(want, nb, N):
        shapes = {"K0": (nb, 2, 4), "K": (nb, N, 2, 4), "dU": (nb, N, 2, 4), "P0": (nb, 10)}
        out = {k: np.zeros(sh) for k, sh in shapes.items() if k in want or k == "K0"}
        if "flag" in want:
            out["flag"] = np.zeros(nb, np.int32)
        return out

    def eval_sens(self, X, U, PI=None, LAM=None, x0=None, t_floor=1e-8, want=("K0",), s0_bound=None):
        """Barrier-smoothed Gauss-Newton sensitivities du_k/dx0 at a point (qsp_eval_sens; definition in
        include/qsp_nmpc.h): a dict with the arrays named in want -- K0 (B, 2, 4) the feedback gain, K (B, N, 2, 4)
        the stage gains, dU (B, N, 2, 4) = du_k/dx0, P0 (B, 10) the value Hessian's upper triangle, flag (B,) 1 on
        a non-finite lane (whose outputs are NaN).  LAM (B, N, 6) as get('lam'); LAM None with PI: the implied
        multipliers of eval_kkt against the handle's references; both None: the unconstrained LQR gains.
        x0 given stands for X's row 0.  s0_bound None: the handle's stage0_s_bound."""
        want = self._sens_want(want)
        B, N = self.B, self.N
        X, U = f64(X, (B, N + 1, 4)), f64(U, (B, N, 2))
        PI = None if PI is None else f64(PI, (B, N, 4))
        LAM = None if LAM is None else f64(LAM, (B, N, 6))
        x0 = None if x0 is None else f64(self._lanes(x0, 4))
        if LAM is None and PI is not None:
            self._rollout_refs(None, None, flush=self._refs_given)
        out = self._sens_outputs(want, B, N)
        o = self._sens_opts(t_floor, s0_bound)
        check(self._L.qsp_eval_sens(self._h, C.byref(o), ptr(x0), ptr(X), ptr(U), ptr(PI), ptr(LAM),
                                    *[ptr(out.get(k)) for k in _lib.SENS_OUTPUTS]), "qsp_eval_sens")
        return {k: out[k] for k in want}

    def eval_sens_device(self, io, t_floor=1e-8, s0_bound=None, stream=None):
        """eval_sens on caller-owned device memory (io: _lib.SensIO of device pointers), asynchronous."""
        o = self._sens_opts(t_floor, s0_bound)
        check(self._L.qsp_eval_sens_device(self._h, C.byref(o), C.byref(io), C.c_void_p(stream) if stream else None),
              "qsp_eval_sens_device")

    def get_sens(self, t_floor=1e-8, want=("K0",), s0_bound=None):
        """eval_sens at the last solve's final, unshifted iterate (qsp_get_sens): its bound multipliers with 'SQP',
        the implied ones with 'SQP_RTI'.  After controller_solve() with 'SQP' only: the RTI path keeps its dynamics
        multipliers only shifted by one stage there, and the call raises QspError (-3)."""
        want = self._sens_want(want)
        out = self._sens_outputs(want, self.B, self.N)
        o = self._sens_opts(t_floor, s0_bound)
        check(self._L.qsp_get_sens(self._h, C.byref(o), *[ptr(out.get(k)) for k in _lib.SENS_OUTPUTS]), "qsp_get_sens")
        return {k: out[k] for k in want}

    def qp_sens(self, A, B, H, want=("K0",)):
        """The sensitivity walk alone on caller-given QP data (qsp_qp_sens): A (nb, N, 16) of qp_solve's structure,
        B (nb, N, 8), H (nb, 6N + 4) diagonal with the barrier terms in it; any horizon N.  A dict as eval_sens."""
        want = self._sens_want(want)
        A = f64(A)
        nb, N = A.shape[0], A.shape[1]
        A, B, H = f64(A, (nb, N, 16)), f64(B, (nb, N, 8)), f64(H, (nb, 6 * N + 4))
        out = self._sens_outputs(want, nb, N)
        check(self._L.qsp_qp_sens(self._h, nb, N, ptr(A), ptr(B), ptr(H), *[ptr(out.get(k)) for k in _lib.SENS_OUTPUTS]),
              "qsp_qp_sens")
        return {k: out[k] for k in want}

    # ------------------------------- rollout costs / u0 cost landscape
    INTEGRATORS ={"euler": 0, "rk4": 1}   # QSP_ROLLOUT_EULER / QSP_ROLLOUT_RK4

    def _rollout_opts(self, integrator, cost_scale):
        if integrator not in self.INTEGRATORS:
            raise ValueError(f"integrator must be one of {tuple(self.INTEGRATORS)}")
        o = _lib.RolloutOpts()
        self._L.qsp_default_rollout_opts(C.byref(o))
        o.integrator = self.INTEGRATORS[integrator]
        o.cost_scale = 1 if cost_scale else 0
        return o

    def _rollout_refs(self, yref, yref_e, flush=True):
        """References of a rollout call: given arrays, or (None) the handle's staged ones -- the last controller
        step's, or what set('cost_y_ref*') holds when that is newer (flushed here, as solve() would; flush=False:
        only what the device already holds)."""
        if flush and (yref is None or yref_e is None) and "yref" in self._dirty and not self._refs_staged:
            check(self._L.qsp_set_yref(self._h, ptr(f64(self._yref)), ptr(f64(self._yref_e))), "qsp_set_yref")
            self._dirty.discard("yref")
        yr = None if yref is None else f64(np.broadcast_to(np.asarray(yref, np.float64), (self.B, self.N, 6)))
        ye = None if yref_e is None else f64(self._lanes(yref_e, 4))
        return yr, ye

    def rollout_cost(self, x0, U, integrator="euler", cost_scale=True, yref=None, yref_e=None, want_viol=False,
                     want_x_end=False):
        """Cost of M control trajectories per lane rolled out from x0 (helper.evaluate_cost_function,
        helper.m:356-367, with the OCP's f): U (B, M, N, 2) -> cost (B, M); with want_viol / want_x_end a
        tuple (cost[, viol (B, M)][, x_end (B, M, 4)]).  cost_scale: stage terms x tau as get_cost (True) or
        unscaled as helper.m:418 (False); yref / yref_e None: the handle's references."""
        x0 = f64(self._lanes(x0, 4))
        U = f64(U)
        if U.ndim != 4 or U.shape[0] != self.B or U.shape[1] < 1 or U.shape[2:] != (self.N, 2):
            raise ValueError(f"U must be (B={self.B}, M >= 1, N={self.N}, 2), got {U.shape}")
        M = U.shape[1]
        o = self._rollout_opts(integrator, cost_scale)
        yr, ye = self._rollout_refs(yref, yref_e)
        cost = np.zeros((self.B, M))
        viol = np.zeros((self.B, M)) if want_viol else None
        xe = np.zeros((self.B, M, 4)) if want_x_end else None
        check(self._L.qsp_rollout_cost(self._h, C.byref(o), M, ptr(x0), ptr(U), ptr(yr), ptr(ye), ptr(cost), ptr(viol),
                                       ptr(xe)), "qsp_rollout_cost")
        out = (cost,) + ((viol,) if want_viol else ()) + ((xe,) if want_x_end else ())
        return out[0] if len(out) == 1 else out

    def cost_landscape(self, x0, un, ut, U_tail=None, integrator="euler", cost_scale=True, yref=None, yref_e=None,
                       want_surface=True):
        """Cost of every first move u_0 = (un[i], ut[j]) with u_k = U_tail[k] for k >= 1, and the grid
        minimiser (helper.debug_cost_function, helper.m:369-431).  U_tail (B, N, 2), row 0 ignored; None: the
        last solve's solution before the controller's shift (ocp_solver.get('u') at helper.m:376).
        Returns dict(cost (B, n_un, n_ut) or None, u_min (B, 2), cost_min (B,), idx_min (B,): 0-based i n_ut + j);
        the first minimum in that order wins, NaN never does (MATLAB's min)."""
        x0 = f64(self._lanes(x0, 4))
        un, ut = f64(un).ravel(), f64(ut).ravel()
        tail = None
        if U_tail is not None:
            tail = f64(np.broadcast_to(np.asarray(U_tail, np.float64), (self.B, self.N, 2)))
        o = self._rollout_opts(integrator, cost_scale)
        yr, ye = self._rollout_refs(yref, yref_e)
        cost = np.zeros((self.B, len(un), len(ut))) if want_surface else None
        u_min, cost_min, idx_min = np.zeros((self.B, 2)), np.zeros(self.B), np.zeros(self.B, np.int32)
        check(self._L.qsp_cost_landscape(self._h, C.byref(o), ptr(x0), ptr(tail), len(un), ptr(un), len(ut), ptr(ut),
                                         ptr(yr), ptr(ye), ptr(cost), ptr(u_min), ptr(cost_min), ptr(idx_min)),
              "qsp_cost_landscape")
        return dict(cost=cost, u_min=u_min, cost_min=cost_min, idx_min=idx_min)

    def rollout_cost_device(self, io, M, integrator="euler", cost_scale=True, stream=None):
        """rollout_cost on caller-owned device memory (io: _lib.RolloutIO of device pointers), asynchronous."""
        o = self._rollout_opts(integrator, cost_scale)
        check(self._L.qsp_rollout_cost_device(self._h, C.byref(o), int(M), C.byref(io),
                                              C.c_void_p(stream) if stream else None), "qsp_rollout_cost_device")

    def cost_landscape_device(self, io, integrator="euler", cost_scale=True, stream=None):
        """cost_landscape on caller-owned device memory (io: _lib.LandscapeIO of device pointers), asynchronous."""
        o = self._rollout_opts(integrator, cost_scale)
        check(self._L.qsp_cost_landscape_device(self._h, C.byref(o), C.byref(io),
                                                C.c_void_p(stream) if stream else None), "qsp_cost_landscape_device")

    # ------------------------------- contact modes / open-loop simulation
    MODES = {0: "", 1: "ST", 2: "SL", 3: "SR"}   # QSP_MODE_*: helper.convert_str2num's coding, 0 = no indicator set
    OPEN_LOOP_OUTPUTS = ("X", "U_out", "S_p", "mode", "mode_steps", "x_end")

    def eval_modes(self, x, u, shape_id=None, want_cone=False):
        """Contact mode of every (x, u) (QSP_MODE_*: 1 sticking, 2 sliding left, 3 sliding right, 0 when
        u_t / u_n is NaN), the branch of f that qsp_eval_dynamics blends.  want_cone: also (n, 3) =
        gamma_l, gamma_r, u_t / u_n."""
        x = f64(x).reshape(-1, 4)
        u = f64(u).reshape(-1, 2)
        n = len(x)
        mode = np.zeros(n, np.int32)
        cone = np.zeros((n, 3)) if want_cone else None
        check(self._L.qsp_eval_modes(self._h, n, ptr(self._sid(shape_id, n)), ptr(x), ptr(u), ptr(mode), ptr(cone)),
              "qsp_eval_modes")
        return (mode, cone) if want_cone else mode

    def get_modes(self, want_cone=False):
        """Stage k's mode at (x_k, u_k) of what get('x') / get('u') return: (B, N)[, cone (B, N, 3)]."""
        mode = np.zeros((self.B, self.N), np.int32)
        cone = np.zeros((self.B, self.N, 3)) if want_cone else None
        check(self._L.qsp_get_modes(self._h, ptr(mode), ptr(cone)), "qsp_get_modes")
        return (mode, cone) if want_cone else mode

    def _open_loop_opts(self, n_steps, M, u_steps, plant_delay, clip, v_alpha, Ts, store_tile):
        o = _lib.OpenLoopOpts()
        self._L.qsp_default_open_loop_opts(C.byref(o))
        o.n_steps, o.M, o.u_steps = int(n_steps), int(M), int(u_steps)
        o.clip, o.v_alpha, o.plant_delay = 1 if clip else 0, float(v_alpha), float(plant_delay)
        o.Ts, o.store_tile = 0.0 if Ts is None else float(Ts), int(store_tile)
        return o

    def open_loop(self, x0, U, n_steps, noise=None, plant_delay=0.0, clip=True, v_alpha=1.0,
                  want=("X", "U_out", "S_p", "mode", "mode_steps"), Ts=None, store_tile=0):
        """helper.open_loop_matlab (helper.m:132-193) for M input candidates per lane.  x0 (B, 4) or (4,);
        U (B, M, 2): held constant, or (B, M, n_steps, 2): replayed; noise (n_steps, B, 4) or None, shared by a
        lane's candidates; plant_delay [s]; clip: u_t <- min(v_alpha / |angle rate|, u_t) (:162-166).
        Returns a dict with x_end (B, M, 4) and the outputs named in `want`: X (B, M, n_steps + 1, 4), U_out
        (B, M, n_steps, 2) the commanded input after the clip, S_p (B, M, n_steps, 2), mode (B, M, n_steps),
        mode_steps (B, M, 4) steps spent in modes 0..3.  Ts None: the handle's; store_tile: include/qsp_nmpc.h."""
        T = int(n_steps)
        x0 = f64(self._lanes(x0, 4))
        U = f64(U)
        if U.ndim == 3 and U.shape[0] == self.B and U.shape[1] >= 1 and U.shape[2] == 2:
            u_steps = 1
        elif U.ndim == 4 and U.shape[0] == self.B and U.shape[1] >= 1 and U.shape[2:] == (T, 2):
            u_steps = T
        else:
            raise ValueError(f"U must be (B={self.B}, M >= 1, 2) or (B={self.B}, M >= 1, n_steps={T}, 2), got {U.shape}")
        unknown = set(want) - set(self.OPEN_LOOP_OUTPUTS)
        if unknown:
            raise KeyError(f"OcpSolver.open_loop: unknown outputs {sorted(unknown)}")
        M = U.shape[1]
        nz = None if noise is None else f64(noise, (T, self.B, 4))
        o = self._open_loop_opts(T, M, u_steps, plant_delay, clip, v_alpha, Ts, store_tile)
        shapes = dict(X=((self.B, M, T + 1, 4), np.float64), U_out=((self.B, M, T, 2), np.float64),
                      S_p=((self.B, M, T, 2), np.float64), mode=((self.B, M, T), np.int32),
                      mode_steps=((self.B, M, 4), np.int32), x_end=((self.B, M, 4), np.float64))
        out = {k: np.zeros(*shapes[k]) for k in self.OPEN_LOOP_OUTPUTS if k in want or k == "x_end"}
        check(self._L.qsp_open_loop(self._h, C.byref(o), ptr(x0), ptr(U), ptr(nz),
                                    *[ptr(out.get(k)) for k in self.OPEN_LOOP_OUTPUTS]), "qsp_open_loop")
        return out

    def open_loop_device(self, io, n_steps, M, u_steps=1, plant_delay=0.0, clip=True, v_alpha=1.0, Ts=None,
                         store_tile=0, stream=None):
        """open_loop on caller-owned device memory (io: _lib.OpenLoopIO of device pointers), asynchronous."""
        o = self._open_loop_opts(n_steps, M, u_steps, plant_delay, clip, v_alpha, Ts, store_tile)
        check(self._L.qsp_open_loop_device(self._h, C.byref(o), C.byref(io), C.c_void_p(stream) if stream else None),
              "qsp_open_loop_device")

    # --------------------------------------------------- controller level
    def set_reference_trajectory(self, traj):
        """traj: 6 x T (MATLAB layout) or T x 6."""
        t = np.asarray(traj, np.float64)
        if t.shape[0] == 6 and t.ndim == 2 and t.shape[1] != 6:
            t = t.T
        t = f64(t)
        if t.ndim != 2 or t.shape[1] != 6:
            raise ValueError("reference trajectory must be 6 x T")
        check(self._L.qsp_set_reference_trajectory(self._h, ptr(t), t.shape[0]), "qsp_set_reference_trajectory")
        self._traj_shape = t.shape

    def set_reference_trajectories(self, traj):
        """Per-lane reference tables: (B, T, 6)."""
        t = f64(traj)
        if t.ndim != 3 or t.shape[0] != self.B or t.shape[2] != 6:
            raise ValueError(f"per-lane references must be (B={self.B}, T, 6), got {t.shape}")
        check(self._L.qsp_set_reference_trajectories(self._h, ptr(t), t.shape[1]), "qsp_set_reference_trajectories")
        self._traj_shape = t.shape

    def gen_straight_lines(self, x0, xf, t0, tf, auto_angle=False):
        """Device-generated TrajectoryGenerator.straight_line per lane (x0, xf: (B, 3)); returns T."""
        a = f64(self._lanes(x0, 3))
        b = f64(self._lanes(xf, 3))
        T = C.c_int32()
        check(self._L.qsp_gen_straight_lines(self._h, ptr(a), ptr(b), float(t0), float(tf), int(bool(auto_angle)),
                                             C.byref(T)), "qsp_gen_straight_lines")
        self._traj_shape = (self.B, T.value, 6)
        return T.value

    def gen_waypoints(self, wp, vel, n_wp=None, law="constant_speed", yaw="heading", theta=None, s_ref=None):
        """Device-generated waypoint paths per lane (qsp_gen_waypoints): TrajectoryGenerator.waypoints_gen
        (law "constant_speed") or waypoint_gen_fixed_angle ("segment_linspace").  wp (B, K, 2) or (K, 2); vel a
        scalar, (K-1,) or (B, K-1), per segment; n_wp (B,) waypoints in use per lane (None: K); yaw "heading",
        "heading_unwrapped" or "fixed" (then theta, a scalar or (B,)); s_ref a scalar or (B,): column 3 of every
        row (None: 0).  Installs the (B, T, 6) tables; returns (T, T_lane): a lane with T_lane < T repeats its
        last row."""
        if law not in _lib.WP_LAWS or yaw not in _lib.WP_YAWS:
            raise ValueError(f"law must be one of {sorted(_lib.WP_LAWS)} and yaw one of {sorted(_lib.WP_YAWS)}")
        w = np.asarray(wp, np.float64)
        if w.ndim == 2:
            w = np.broadcast_to(w, (self.B,) + w.shape)
        if w.ndim != 3 or w.shape[0] != self.B or w.shape[2] != 2:
            raise ValueError(f"wp must be (B={self.B}, K, 2) or (K, 2), got {w.shape}")
        K = w.shape[1]
        w = f64(w)
        v = f64(np.broadcast_to(np.asarray(vel, np.float64), (self.B, max(K - 1, 1))))

        def lanes(a, dtype):
            return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype), (self.B,)))

        n, th, sr = lanes(n_wp, np.int32), lanes(theta, np.float64), lanes(s_ref, np.float64)
        o = _lib.WaypointOpts()
        self._L.qsp_default_waypoint_opts(C.byref(o))
        o.law, o.yaw = _lib.WP_LAWS[law], _lib.WP_YAWS[yaw]
        T = C.c_int32()
        Tl = np.zeros(self.B, np.int32)
        check(self._L.qsp_gen_waypoints(self._h, C.byref(o), K, ptr(w), ptr(n), ptr(v), ptr(th), ptr(sr), C.byref(T),
                                        ptr(Tl)), "qsp_gen_waypoints")
        self._traj_shape = (self.B, T.value, 6)
        return T.value, Tl

    def get_reference_trajectories(self):
        out = np.zeros(self._traj_shape)
        check(self._L.qsp_get_reference_trajectories(self._h, ptr(out)), "qsp_get_reference_trajectories")
        return out

    def controller_solve(self, x0, index_time):
        x0 = f64(self._lanes(x0, 4))
        idx = i32(np.broadcast_to(np.asarray(index_time, np.int32), (self.B,)))
        self._timed(lambda: check(self._L.qsp_controller_solve(self._h, ptr(x0), ptr(idx)), "qsp_controller_solve"))
        self._refs_staged = True
        return self.get_u0()

    def _closed_loop_args(self, x0, n_steps, index0, noise, plant_delay, disturbance, t_dist, amplitude):
        """The two closed-loop entries' common arguments; the amplitude array is returned to keep it alive."""
        n = int(n_steps)
        x0 = f64(self._lanes(x0, 4))
        idx = i32(np.broadcast_to(np.asarray(index0, np.int32), (self.B,)))
        nz = None if noise is None else f64(noise, (n, self.B, 4))
        amp = None if amplitude is None else f64(np.broadcast_to(np.asarray(amplitude, np.float64), (self.B,)))
        o = _lib.ClosedLoopOpts()
        o.plant_delay, o.disturbance, o.t_dist = float(plant_delay), 1 if disturbance else 0, int(t_dist)
        o.amplitude = None if amp is None else amp.ctypes.data
        return n, x0, idx, nz, o, amp

    METRICS = ("sum_exy2", "max_exy2", "sum_eth2", "end_exy2", "sum_u2", "n_failed", "n_st", "n_sl", "n_sr",
               "n_s_out")   # QSP_CLM_* (include/qsp_nmpc.h)

    def closed_loop_metrics(self, x0, n_steps, index0=1, noise=None, plant_delay=0.0, disturbance=False, t_dist=0,
                            amplitude=None):
        """closed_loop's run reduced on the device to per-lane metrics (qsp_closed_loop_metrics): no trajectory
        is kept or copied.  Returns dict(metrics (B, 10), one (B,) column under each name of METRICS, x_end
        (B, 4) the state after the last plant step, status (B,) the last solve's).  The tracking errors are
        against the installed reference table at column index0 + i - 1, clamped at its end."""
        n, x0, idx, nz, o, _amp = self._closed_loop_args(x0, n_steps, index0, noise, plant_delay, disturbance, t_dist,
                                                         amplitude)
        m = np.zeros((self.B, len(self.METRICS)))
        xe = np.zeros((self.B, 4))
        st = np.zeros(self.B, np.int32)
        check(self._L.qsp_closed_loop_metrics(self._h, C.byref(o), ptr(x0), ptr(idx), n, ptr(nz), ptr(m), ptr(xe),
                                              ptr(st)), "qsp_closed_loop_metrics")
        self._refs_staged = True
        out = dict(metrics=m, x_end=xe, status=st)
        out.update({k: m[:, j] for j, k in enumerate(self.METRICS)})
        return out

    def closed_loop(self, x0, n_steps, index0=1, noise=None, plant_delay=0.0, disturbance=False, t_dist=0,
                    amplitude=None):
        """Device-resident closed loop (helper.m:195-322): returns X (B, n+1, 4) (plant states after
        disturbance and noise), Xsim (B, n, 4) (the delay-predicted states the solver sees), U (B, n, 2),
        status (B, n).  noise: (n, B, 4) additive state noise before each solve, or None (then drawn on the
        device where set_sim_noise installed a generator); plant_delay [s];
        disturbance at the 1-based step t_dist with per-lane amplitude (y offset + contact re-projection)."""
        n, x0, idx, nz, o, _amp = self._closed_loop_args(x0, n_steps, index0, noise, plant_delay, disturbance, t_dist,
                                                         amplitude)
        X = np.zeros((self.B, n + 1, 4))
        Xs = np.zeros((self.B, n, 4))
        U = np.zeros((self.B, n, 2))
        st = np.zeros((self.B, n), np.int32)
        check(self._L.qsp_closed_loop_ex(self._h, C.byref(o), ptr(x0), ptr(idx), n, ptr(nz), ptr(X), ptr(Xs), ptr(U),
                                         ptr(st)), "qsp_closed_loop_ex")
        self._refs_staged = True
        return dict(X=X, Xsim=Xs, U=U, status=st)

    # ------------------------------------------------ delay compensation
    def set_delay_comp(self, delay):
        """set_delay_comp (NMPC_controller.m:106-110): delay_buff_comp = ceil(delay / Ts)."""
        check(self._L.qsp_set_delay_comp(self._h, float(delay)), "qsp_set_delay_comp")

    def delay_cols(self):
        d = C.c_int32()
        check(self._L.qsp_get_delay_comp(self._h, C.byref(d)), "qsp_get_delay_comp")
        return d.value

    def delay_buffer_sim(self, x):
        """delay_buffer_sim (NMPC_controller.m:112-120) on the device, per lane."""
        x = f64(self._lanes(x, 4))
        out = np.zeros((self.B, 4))
        check(self._L.qsp_delay_buffer_sim(self._h, ptr(x), ptr(out)), "qsp_delay_buffer_sim")
        return out

    def delay_buffer_push(self, u):
        """u_buff_contr = [u, u_buff_contr(:, 1:end-1)] (helper.m:255)."""
        u = f64(self._lanes(u, 2))
        check(self._L.qsp_delay_buffer_push(self._h, ptr(u)), "qsp_delay_buffer_push")

    def reproject_contact(self, px, py, s0, shape_id=None):
        px = f64(px).ravel()
        n = len(px)
        py = f64(np.broadcast_to(py, (n,)))
        s0 = f64(np.broadcast_to(s0, (n,)))
        out = np.zeros(n)
        check(self._L.qsp_reproject_contact(self._h, n, ptr(self._sid(shape_id, n)), ptr(px), ptr(py), ptr(s0),
                                            ptr(out)), "qsp_reproject_contact")
        return out

    def controller_reset(self):
        check(self._L.qsp_controller_reset(self._h), "qsp_controller_reset")

    # --------------------------------------------------------- device path
    def solve_device(self, io, stream=None):
        check(self._L.qsp_solve_device(self._h, C.byref(io), C.c_void_p(stream) if stream else None), "qsp_solve_device")

    def synchronize(self):
        check(self._L.qsp_synchronize(self._h), "qsp_synchronize")

    def set_stream_parts(self, parts):
        """SQP loop in 1 or 2 parts on their own HIP streams (0 = auto); results are identical."""
        check(self._L.qsp_set_stream_parts(self._h, int(parts)), "qsp_set_stream_parts")

    def stream_parts(self):
        p = C.c_int32()
        check(self._L.qsp_get_stream_parts(self._h, C.byref(p)), "qsp_get_stream_parts")
        return p.value

    def set_kernel_timing(self, max_solves):
        """Record HIP events at every kernel boundary of the next `max_solves` solves."""
        check(self._L.qsp_set_kernel_timing(self._h, int(max_solves)), "qsp_set_kernel_timing")

    KERNELS = ("prologue", "linearize", "qp_step", "epilogue")

    def kernel_times(self):
        """{kernel: (total_ms, launches)} over the timed solves since the last call."""
        ms = (C.c_double * 4)()
        n = (C.c_int32 * 4)()
        check(self._L.qsp_get_kernel_times(self._h, ms, n), "qsp_get_kernel_times")
        return {k: (ms[i], n[i]) for i, k in enumerate(self.KERNELS)}

    # ----------------------------------------------------- building blocks
    def _sid(self, shape_id, n):
        return i32(np.broadcast_to(np.asarray(0 if shape_id is None else shape_id, np.int32), (n,)))

    def eval_spline(self, sigma, shape_id=None):
        s = f64(sigma).ravel()
        n = len(s)
        Cv, D, Dd, kap = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
        check(self._L.qsp_eval_spline(self._h, n, ptr(self._sid(shape_id, n)), ptr(s), ptr(Cv), ptr(D), ptr(Dd),
                                      ptr(kap)), "qsp_eval_spline")
        return Cv, D, Dd, kap

    def eval_dynamics(self, x, u, shape_id=None):
        x = f64(x).reshape(-1, 4)
        u = f64(u).reshape(-1, 2)
        n = len(x)
        f, J = np.zeros((n, 4)), np.zeros((n, 4, 6))
        check(self._L.qsp_eval_dynamics(self._h, n, ptr(self._sid(shape_id, n)), ptr(x), ptr(u), ptr(f), ptr(J)),
              "qsp_eval_dynamics")
        return f, J

    def eval_rk4(self, x, u, h=None, shape_id=None):
        x = f64(x).reshape(-1, 4)
        u = f64(u).reshape(-1, 2)
        n = len(x)
        xn, A, Bm = np.zeros((n, 4)), np.zeros((n, 4, 4)), np.zeros((n, 4, 2))
        check(self._L.qsp_eval_rk4(self._h, n, ptr(self._sid(shape_id, n)), self.Ts if h is None else h, ptr(x),
                                   ptr(u), ptr(xn), ptr(A), ptr(Bm)), "qsp_eval_rk4")
        return xn, A, Bm

    def eval_vbound(self, s, shape_id=None):
        s = f64(s).ravel()
        n = len(s)
        vb = np.zeros(n)
        check(self._L.qsp_eval_vbound(self._h, n, ptr(self._sid(shape_id, n)), ptr(s), ptr(vb)), "qsp_eval_vbound")
        return vb

    def qp_solve(self, A, B, b, H, g, lo, hi, dx0):
        N = self.N
        nb = A.shape[0]
        arrs = [f64(a) for a in (A, B, b, H, g, lo, hi, dx0)]
        dx, du = np.zeros((nb, N + 1, 4)), np.zeros((nb, N, 2))
        pi, lam = np.zeros((nb, N, 4)), np.zeros((nb, N, 6))
        iters = np.zeros(nb, np.int32)
        qst = np.zeros(nb, np.int32)
        check(self._L.qsp_qp_solve(self._h, nb, *[ptr(a) for a in arrs], ptr(dx), ptr(du), ptr(pi), ptr(lam),
                                   ptr(iters), ptr(qst)), "qsp_qp_solve")
        return dict(dx=dx, du=du, pi=pi, lam=lam, iters=iters, qp_status=qst)

    def qp_residuals(self, A, B, b, H, g, lo, hi, dx0, dx, du, pi, lam):
        """KKT residuals of QP points recomputed on the device (qsp_qp_residuals): qp_solve's array layouts,
        none of its restrictions on H, the bound widths or A.  Returns a dict of (nb,) arrays keyed
        _lib.QP_RESIDUALS (stat_u, stat_x, dyn, infeas, comp, dual); the stage-0 s row counts in the last
        three with stage0_s_bound only."""
        N = self.N
        nb = np.shape(b)[0]
        shapes = ((nb, N, 16), (nb, N, 8), (nb, N, 4), (nb, 6 * N + 4), (nb, 6 * N + 4), (nb, N, 3), (nb, N, 3), (nb, 4),
                  (nb, N + 1, 4), (nb, N, 2), (nb, N, 4), (nb, N, 6))
        arrs = [f64(a, sh) for a, sh in zip((A, B, b, H, g, lo, hi, dx0, dx, du, pi, lam), shapes)]
        res = np.zeros((nb, len(_lib.QP_RESIDUALS)))
        check(self._L.qsp_qp_residuals(self._h, nb, *[ptr(a) for a in arrs], ptr(res)), "qsp_qp_residuals")
        return {k: res[:, i].copy() for i, k in enumerate(_lib.QP_RESIDUALS)}
