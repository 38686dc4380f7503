"""
Dense-link models (BASELINE config 4): lowering and engine for graphs whose likelihood goes through
``BF.matmul(weights, x)`` with a random minibatch ``x``.

The scalar fused kernel keeps one latent *scalar* per LDS slot; a 10x784 weight matrix per sample
does not belong there.  This module recognises the reference's Bayesian logistic-regression shape
(`examples/MNIST_logistic_regression.py:15-54`, `examples/minibatch_logistic_regression.py:13-51`)

    indices = RandomIndices(dataset_size, batch_size, "indices", is_observed=True)
    x       = EmpiricalVariable(X,      indices=indices, name="x",      is_observed=True)
    labels  = EmpiricalVariable(labels, indices=indices, name="labels", is_observed=True)
    weights = NormalVariable(loc0, scale0, "weights")
    k       = CategoricalVariable(logits=BF.matmul(weights, x), name="k");  k.observe(labels)
    q:        NormalVariable(loc, scale, "weights", learnable=True)

and hands it to the MFMA kernels of `csrc/dense_kernel.inc` through `bsvi_dense_*` (include/bsvi.h).
The reference's semantics are kept, including the name-collision rule that makes the prior's
`weights_loc` / `weights_scale` the posterior's own roots and the absence of any
minibatch rescaling of the likelihood (`variables.py:849` TODO).
"""
import ctypes as C

import numpy as np
import torch

from brancher_amd import distributions as D
from brancher_amd import lowering, native
from brancher_amd.lowering import LoweringError, _Lowering
from brancher_amd.native import OUT_HEADER
from brancher_amd.variables import RandomVariable, RootVariable

LIK_CATEGORICAL, LIK_BERNOULLI = 0, 1


from brancher_amd.native import DenseDesc, DenseArgs


class DenseProgram:
    """What `lower_dense` extracts from the graph."""
    estimator = "pathwise"

    def summary(self):
        return dict(kind="dense", n_classes=self.n_classes, n_features=self.n_features,
                    dataset_size=self.dataset_size, batch_size=self.batch_size, n_params=self.n_params,
                    likelihood=("categorical", "bernoulli")[self.likelihood], latent=self.latent_name)


def _is_random(v):
    return isinstance(v, RandomVariable) and getattr(v, "_type", None) != "Deterministic node"


def lower_dense(joint, posterior, estimator="pathwise"):
    if estimator not in ("pathwise", "blackbox", "local"):
        raise LoweringError("the dense-link path implements the Pathwise, BlackBox and LocalReparameterization estimators, not %r" % (estimator,))
    L = _Lowering(joint, posterior, estimator)
    q_flat = posterior._flatten()
    L.q_by_name = {v.name: v for v in q_flat}
    L.q_roots = {v for v in posterior.variables if isinstance(v, RootVariable)}
    for v in sorted(L.q_roots, key=lambda v: v.name):
        if v.learnable:
            L.param_offset(v.parameter, 0)
    for v in sorted([v for v in joint.flatten() if isinstance(v, RootVariable)], key=lambda v: v.name):
        if v.learnable:
            L.param_offset(v.parameter, 1)

    q_random = [v for v in q_flat if _is_random(v)]
    # point estimate (MAP, inference.py:251-275; examples/MAP_logistic_regression.py:46-56): the posterior is ONE
    # learnable RootVariable carrying the weight variable's name -> W = its value, no noise, no entropy
    point = None
    if not q_random:
        roots = [v for v in q_flat if isinstance(v, RootVariable) and v.learnable]
        if len(roots) == 1:
            point = roots[0]
    if point is None and (len(q_random) != 1 or q_random[0].distribution.kind != D.DIST_NORMAL):
        raise LoweringError("dense path: the posterior must be one mean-field Normal weight variable "
                            "(or one learnable RootVariable: a point estimate)")
    if point is not None and estimator == "local":
        raise LoweringError("dense path: the 'local' estimator reparameterises a Normal posterior; %r is a point estimate: use Pathwise "
                            "or MAP" % point.name)
    Wq = point if point is not None else q_random[0]
    p_random = [v for v in joint._flatten() if _is_random(v)]
    liks = [v for v in p_random if v.distribution.kind in (D.DIST_CATEGORICAL, D.DIST_BINOMIAL, D.DIST_BERNOULLI)]
    weights = [v for v in p_random if v.name == Wq.name and v.distribution.kind == D.DIST_NORMAL]
    others = [v for v in p_random if v not in liks and v not in weights and v.distribution.kind != D.DIST_EMPIRICAL]
    if len(liks) != 1 or len(weights) != 1 or others:
        raise LoweringError("dense path: expected one weight prior and one matmul likelihood")
    k, Wp = liks[0], weights[0]
    if not k.is_observed or not k.has_random_dataset:
        raise LoweringError("dense path: the likelihood must be observed through an EmpiricalVariable of labels")
    links = k.link.expressions()
    if "logits" not in links:
        raise LoweringError("dense path: the likelihood must be parameterised by logits")
    e = links["logits"].expr
    if not (e.op == "call" and e.attr[0] == "matmul" and len(e.args) == 2 and all(a.op == "var" for a in e.args)):
        raise LoweringError("dense path: logits must be BF.matmul(weights, x)")
    w_var, x_var = e.args[0].attr, e.args[1].attr
    if w_var is not Wp:
        raise LoweringError("dense path: the first matmul operand must be the weight variable")
    labels_var = k.dataset

    def minibatch_source(v, what):
        if getattr(v, "_type", None) != "Empirical" or not v.is_observed:
            raise LoweringError("dense path: %s must be an observed EmpiricalVariable" % what)
        exprs = v.link.expressions()
        ds = exprs["dataset"].expr
        if ds.op != "var" or not isinstance(ds.attr, RootVariable) or "indices" not in exprs:
            raise LoweringError("dense path: %s must index an array dataset through a RandomIndices variable" % what)
        ind = exprs["indices"].expr
        from brancher_amd.standard_variables import RandomIndices
        if ind.op != "var" or not isinstance(ind.attr, RandomIndices):
            raise LoweringError("dense path: %s must be indexed by a RandomIndices variable" % what)
        return np.asarray(ds.attr.value, dtype=np.float32), ind.attr

    X, ind_x = minibatch_source(x_var, "x")
    Y, ind_y = minibatch_source(labels_var, "labels")
    if ind_x is not ind_y:
        raise LoweringError("dense path: x and labels must share one RandomIndices variable")
    # observed datasets are stored as [1, DS, P, 1] / [1, DS, 1, 1] (utilities.py:226-232)
    DS = X.shape[1]
    Xm = X.reshape(DS, -1)
    Ym = Y.reshape(-1)
    if Ym.shape[0] != DS:
        raise LoweringError("dense path: dataset sizes of x and labels differ")
    P = Xm.shape[1]
    batch = int(ind_x.batch_size)

    # -- weight parameters through the uniform table
    def row_params(var, ctx):
        out = []
        for node in L.node_params(var, ctx):
            m = L.match_uniform(node)
            if m is None:
                raise LoweringError("dense path: the parameters of %r must be constants or parameter transforms" % var.name)
            leaf, g, a, b = m
            is_param, k0 = L.uniform_entries(leaf, g, a, b)
            size = int(np.prod(leaf.shape))
            out.append((is_param, k0, size, leaf.shape))
        return out

    if point is not None:
        leaf = L.q_value(point)
        is_param, k0 = L.uniform_entries(leaf, "identity", 0.0, 1.0)
        ql = (is_param, k0, int(np.prod(leaf.shape)), leaf.shape)
        _, z0 = L.const_operand(0.0)                         # scale 0: W = loc exactly, whatever the noise
        qs = (False, z0, 1, (1, 1, 1))
    else:
        (ql, qs) = row_params(Wq, L.q_value)
    (pl, ps) = row_params(Wp, L.p_value)
    shape = ql[3]
    C_, P_ = shape[1], shape[2]
    if shape[0] != 1 or P_ != P or ql[2] != C_ * P_:
        raise LoweringError("dense path: weights of shape %r do not match %d features" % (shape, P))
    lik = LIK_CATEGORICAL if k.distribution.kind == D.DIST_CATEGORICAL else LIK_BERNOULLI
    if lik == LIK_BERNOULLI:
        if C_ != 1:
            raise LoweringError("dense path: a Bernoulli/Binomial likelihood needs a single output")
        if k.distribution.kind == D.DIST_BINOMIAL:
            tc = L.match_uniform(L.from_expr(links["total_count"].expr, L.p_value))
            if tc is None or tc[0].op != "root" or float(np.asarray(tc[0].attr.value).reshape(-1)[0]) != 1.0:
                raise LoweringError("dense path: Binomial likelihood supports total_count = 1 only")

    uni, n_up = L.uniform_table()
    prog = DenseProgram()
    prog.estimator = estimator
    L.fill_parameter_tables(prog, uni, n_up)

    def base(entry):
        is_param, k0, size, _ = entry
        return (k0 if is_param else n_up + k0), (1 if size > 1 else 0)

    prog.uniform = uni
    prog.consts = np.concatenate(L.consts) if L.consts else np.zeros(0, np.float32)
    prog.q_loc, prog.q_scale, prog.prior_loc, prog.prior_scale = base(ql), base(qs), base(pl), base(ps)
    for b_, size in ((ql, 0), (qs, 0), (pl, 0), (ps, 0)):
        if b_[2] not in (1, C_ * P_):
            raise LoweringError("dense path: a weight parameter has an unsupported shape")
    prog.n_classes, prog.n_features, prog.dataset_size, prog.batch_size = C_, P_, DS, batch
    prog.likelihood = lik
    prog.dataset = np.ascontiguousarray(Xm, dtype=np.float32)
    prog.labels = np.ascontiguousarray(Ym, dtype=np.float32)
    prog.latent_name = Wq.name
    prog.point_estimate = point is not None
    prog.indices_name = ind_x.name
    prog.x_name, prog.likelihood_name = x_var.name, k.name
    prog.lik_weight, prog.prior_weight, prog.entropy_weight = 1.0, 1.0, (0.0 if point is not None else 1.0)
    prog.n_noise = C_ * P_
    prog.bmax = 1
    return prog


MIN_PARTICLES, MAX_PARTICLES, MAX_PARTICLE_CLASSES, MAX_PARTICLE_FEATURES = 2, 256, 32, 1024


def check_particles(p, n_particles):
    """what `bsvi_dense_particles_fwd_bwd` serves, asked of a lowered program before any device work (the library asks the same of its
    handle); every refusal is a ValueError that names the feature or the limit"""
    where = "batched particles (bsvi_dense_particles_fwd_bwd): "
    if not MIN_PARTICLES <= n_particles <= MAX_PARTICLES:
        raise ValueError(where + "{} particles, served are {} .. {}".format(n_particles, MIN_PARTICLES, MAX_PARTICLES))
    if not p.point_estimate:
        raise ValueError(where + "{} has a Normal posterior (a particle is a model of one learnable RootVariable named like the "
                                 "weights: a point estimate)".format(p.latent_name))
    if p.n_classes > MAX_PARTICLE_CLASSES:
        raise ValueError(where + "{} classes, served are 1 .. {}".format(p.n_classes, MAX_PARTICLE_CLASSES))
    if p.n_features > MAX_PARTICLE_FEATURES:
        raise ValueError(where + "{} features, served are 1 .. {}".format(p.n_features, MAX_PARTICLE_FEATURES))


def row_parameters(p, theta=None):
    """(q loc [C P], q scale [C P]) of a lowered program at the flat parameter values `theta`: the uniform table on the host, in
    double precision (`bnn.row_parameters` on this path's two row ranges) — what `dense_predict_head` leaves in `rowp` on the device"""
    import types
    from brancher_amd import bnn
    rows = np.arange(p.n_classes * p.n_features)
    shim = types.SimpleNamespace(uniform=p.uniform, consts=p.consts, parameters=p.parameters, n_params=p.n_params,
                                 row_uniform=(p.q_loc[0] + p.q_loc[1] * rows, p.q_scale[0] + p.q_scale[1] * rows))
    return bnn.row_parameters(shim, theta)


class CompiledDense:
    """Engine for a dense-link model; same surface as engine.CompiledELBO."""

    def data_path(self):
        """which matrix-core path serves the two products of an iteration: "bf16x3" when every dataset value is exactly a
        bf16 number (three bf16 MFMAs on the exact pieces of the f32 operand, bsvi_dense_exact_data), else "f32" """
        return "bf16x3" if self._exact_data else "f32"

    def launch_plan(self, number_samples, noise=False, want_fvalues=False, weighted=False):
        """the kernels an evaluation of `number_samples` samples launches, by name and in order, without launching them
        (bsvi_dense_plan; csrc/dense_select.h): `noise` — the caller supplies the normals; `want_fvalues` — per-sample values
        (and log q under the BlackBox estimator) are asked for, as `evaluate` does; `weighted` — `evaluate_weighted`"""
        from brancher_amd import engine
        if self._local():
            raise ValueError("launch_plan: the 'local' estimator has a launch sequence of its own (bsvi_dense_local_fwd_bwd: dense_head, "
                             "dense_local_fwd, dense_local_join, dense_local_bwd, dense_local_tail, dense_param_kernel), not a plan of "
                             "bsvi_dense_plan")
        rank, world = engine.dist_info()
        _, n_local = engine.shard(number_samples, rank, world)
        some = lambda present: C.c_void_p(16) if present else None      # only the presence of an optional pointer matters
        blackbox = getattr(self.program, "estimator", "pathwise") == "blackbox"
        args = DenseArgs(n_samples_local=n_local, n_samples_global=number_samples, noise_dev=some(noise),
                         fvalue_out_dev=some(want_fvalues), logq_out_dev=some(want_fvalues and blackbox),
                         f_weight_dev=some(weighted), q_weight_dev=some(weighted))
        kinds = (C.c_int32 * 16)()
        n = self.lib.bsvi_dense_plan(self.handle, C.byref(args), kinds, 16)
        if n < 0:
            native.check(n)
        return [self.lib.bsvi_dense_kind_name(kinds[i]).decode() for i in range(n)]

    def __init__(self, joint_model, posterior_model, estimator="pathwise", device=None, program=None, particles=False):
        from brancher_amd import engine
        self.device = device or engine._device()
        self.program = program if program is not None else lower_dense(joint_model, posterior_model, estimator)
        p = self.program
        lib = native.load()
        if lib.bsvi_device_count() < 1:
            raise native.NativeError("no MI355X / HIP device visible: the engine cannot run (no CPU fallback)")
        self.lib = lib
        self._keep = dict(uniform=np.ascontiguousarray(p.uniform), consts=np.ascontiguousarray(p.consts, dtype=np.float32),
                          ptr=np.ascontiguousarray(p.param_uniform_ptr, dtype=np.uint32),
                          idx=np.ascontiguousarray(p.param_uniform_idx, dtype=np.uint32),
                          dataset=p.dataset, labels=p.labels)
        k = self._keep
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        d = DenseDesc(abi_version=native.ABI_VERSION, n_params=p.n_params, n_consts=k["consts"].size,
                      n_uniform=len(k["uniform"]), n_uniform_grad=p.n_uniform_grad,
                      n_classes=p.n_classes, n_features=p.n_features, dataset_size=p.dataset_size,
                      batch_size=p.batch_size, likelihood=p.likelihood,
                      q_loc_u=p.q_loc[0], q_scale_u=p.q_scale[0], prior_loc_u=p.prior_loc[0], prior_scale_u=p.prior_scale[0],
                      q_loc_stride=p.q_loc[1], q_scale_stride=p.q_scale[1], prior_loc_stride=p.prior_loc[1],
                      prior_scale_stride=p.prior_scale[1], lik_weight=p.lik_weight, prior_weight=p.prior_weight,
                      entropy_weight=p.entropy_weight, estimator=lowering.EST[getattr(p, "estimator", "pathwise")],
                      uniform=ptr(k["uniform"]), consts=ptr(k["consts"]),
                      param_uniform_ptr=ptr(k["ptr"]), param_uniform_idx=ptr(k["idx"]), dataset=ptr(k["dataset"]),
                      labels=ptr(k["labels"]))
        if p.n_classes > 16 and not particles:      # the library creates 17 .. 32 classes for bsvi_dense_particles_fwd_bwd alone
            raise native.NativeError("dense path supports at most 16 classes")
        handle = C.c_void_p()
        native.check(lib.bsvi_dense_create(C.byref(d), C.byref(handle)))
        self.handle = handle
        self._exact_data = bool(lib.bsvi_dense_exact_data(handle))
        dev = self.device
        self.n_params = p.n_params
        theta = np.zeros(p.n_params, dtype=np.float32)
        for par, off, size, _ in p.parameters:
            theta[off:off + size] = par.numpy().reshape(-1)
        self.params = _engine.broadcast_from_rank0(torch.from_numpy(theta).to(dev))
        self.out = torch.zeros(OUT_HEADER + max(p.n_params, 1), device=dev)
        active = np.ascontiguousarray(p.param_active, dtype=np.uint8)
        group = p.param_group
        first_group = 0 if np.any(active[group == 0]) else 1
        self.mask_all = torch.from_numpy(active.copy()).to(dev)
        self.mask_first = torch.from_numpy((active * (group == first_group)).astype(np.uint8)).to(dev)
        self._workspaces = {}
        self.iteration = 0
        self.grads_valid = False
        self.last_mode = None
        for par, off, size, _ in p.parameters:
            par.bind(self, off)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.bsvi_dense_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ParameterStore protocol
    def read_params(self, offset, size):
        return self.params[offset:offset + size].detach().cpu().numpy()

    def write_params(self, offset, values):
        self.params[offset:offset + values.size] = torch.from_numpy(np.ascontiguousarray(values)).to(self.device)

    def read_grads(self, offset, size):
        if not self.grads_valid:
            return None
        o = OUT_HEADER + offset
        return self.out[o:o + size].detach().cpu().numpy()

    def workspace(self, n_local):
        ws = self._workspaces.get(n_local)
        if ws is None:
            ws = torch.empty(int(self.lib.bsvi_dense_workspace_bytes(self.handle, n_local)), dtype=torch.uint8,
                             device=self.device)
            self._workspaces[n_local] = ws
        return ws

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _seed(self, seed):
        return _engine.shared_seed(seed, self.device)

    def _args(self, n_local, n_global, base, noise=None, indices=None, seed=None, offset=0, noise_out=None,
              indices_out=None, fvalue_out=None, f_weight=None, q_weight=None, logq_out=None):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        seed = _engine.shared_seed(seed, self.device)
        return DenseArgs(params_dev=ptr(self.params), noise_dev=ptr(noise), indices_dev=ptr(indices), seed=seed,
                         offset=int(offset), n_samples_local=n_local, n_samples_global=n_global, sample_base=base,
                         out_dev=ptr(self.out), noise_out_dev=ptr(noise_out), indices_out_dev=ptr(indices_out),
                         fvalue_out_dev=ptr(fvalue_out), workspace_dev=ptr(self.workspace(n_local)), stream=self._stream(),
                         f_weight_dev=ptr(f_weight), q_weight_dev=ptr(q_weight), logq_out_dev=ptr(logq_out))

    def _noise_tensor(self, noise, n_global, base, n_local):
        if noise is None:
            return None
        if isinstance(noise, dict):
            if self.program.point_estimate and self.program.latent_name not in noise:
                return None                  # nothing is sampled: the weights' scale is 0, any noise gives W = loc
            a = np.asarray(noise[self.program.latent_name], dtype=np.float32)       # [N, 1, C, P]
            noise = np.ascontiguousarray(a.reshape(a.shape[0], -1).T)               # [C*P, N]
        if isinstance(noise, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(noise[:, base:base + n_local], dtype=np.float32)).to(self.device)
        return noise if noise.shape[1] == n_local else noise[:, base:base + n_local].contiguous()

    def _indices_tensor(self, minibatch):
        if minibatch is None:
            return None
        if isinstance(minibatch, dict):
            minibatch = minibatch[self.program.indices_name]
        return torch.as_tensor(np.asarray(minibatch, dtype=np.int32)).to(self.device)

    def evaluate(self, number_samples, noise=None, minibatch=None, seed=None, offset=None, want_noise=False,
                 want_fvalues=False, want_indices=False, **_):
        from brancher_amd import engine
        if self._local():
            if want_fvalues:
                raise ValueError("the 'local' estimator has no per-sample f values (want_fvalues): its prior and entropy terms are closed "
                                 "forms, not sums over samples")
            return self._evaluate_local(number_samples, noise, minibatch, seed, offset, want_noise, want_indices)
        rank, world = engine.dist_info()
        base, n_local = engine.shard(number_samples, rank, world)
        if n_local == 0:
            raise ValueError("number_samples={} is smaller than the number of GPUs {}".format(number_samples, world))
        if offset is None:
            offset = self.iteration
            self.iteration += 1
        dev, p = self.device, self.program
        noise_t = self._noise_tensor(noise, number_samples, base, n_local)
        idx_t = self._indices_tensor(minibatch)
        noise_o = torch.empty((p.n_noise, n_local), device=dev) if want_noise else None
        idx_o = torch.empty(p.batch_size, device=dev, dtype=torch.int32) if want_indices else None
        fvals = torch.empty(n_local, device=dev) if want_fvalues else None
        # (per-sample log q next to per-sample f: what a BlackBox-style estimator multiplies — a point estimate has no q)
        logq = torch.zeros(n_local, device=dev) if want_fvalues and getattr(p, "estimator", "pathwise") == "blackbox" else None
        args = self._args(n_local, number_samples, base, noise_t, idx_t, seed, offset, noise_o, idx_o, fvals, logq_out=logq)
        native.check(self.lib.bsvi_dense_fwd_bwd(self.handle, C.byref(args)))
        engine.allreduce_sums(self.out)
        engine.check_exchange(self.device, self.params)
        native.check(self.lib.bsvi_dense_finalize(self.handle, C.c_void_p(self.out.data_ptr()), number_samples, self._stream()))
        self.grads_valid = True
        res = dict(loss=self.out[2], finite=self.out[3], nonfinite_count=self.out[1],
                   grads=self.out[OUT_HEADER:OUT_HEADER + p.n_params], n_local=n_local, sample_base=base)
        if want_noise:
            res["noise"] = noise_o
        if want_indices:
            res["indices"] = idx_o
        if want_fvalues:
            res["f"] = fvals
            if logq is not None:
                res["lq"] = logq
        return res

    # ---- the local reparameterisation estimator (program.estimator == "local": bsvi_dense_local_fwd_bwd, csrc/dense_local.inc)
    def _local(self):
        return getattr(self.program, "estimator", "pathwise") == "local"

    def _local_args(self, N, seed, offset):
        """the argument struct of a call of N samples (the caller fills in noise, indices and slots), with the workspace of that N"""
        from brancher_amd import engine
        if engine.dist_info()[1] > 1:
            raise ValueError("the 'local' estimator runs on one GPU: its samples are not sharded over ranks (world size {})".format(
                engine.dist_info()[1]))
        # asked on every call: the plan reads BSVI_LOCAL_SPLITS per call, and more splits need more of dM / dV than the cached block has
        need = int(self.lib.bsvi_dense_local_workspace_bytes(self.handle, N))
        if need == 0:
            native.check(-1)
        ws = self._workspaces.get(("local", N))
        if ws is None or ws.numel() < need:
            ws = self._workspaces[("local", N)] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return native.DenseLocalArgs(n_samples=N, params_dev=self.params.data_ptr(), out_dev=self.out.data_ptr(), workspace_dev=ws.data_ptr(),
                                     stream=self._stream(), seed=_engine.shared_seed(seed, self.device), offset=int(offset))

    def _local_noise(self, noise, N):
        """the caller's zeta as a contiguous f32 device tensor [N, B, C]: an array, or {likelihood name: array}"""
        if noise is None:
            return None
        p = self.program
        if isinstance(noise, dict):
            if p.likelihood_name not in noise:
                raise ValueError("the 'local' estimator draws the logits of {!r}: its noise is {{{!r}: [N, B, C]}} (the weights are never "
                                 "drawn)".format(p.likelihood_name, p.likelihood_name))
            noise = noise[p.likelihood_name]
        t = noise if torch.is_tensor(noise) else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32))
        if tuple(t.shape) != (N, p.batch_size, p.n_classes):
            raise ValueError("noise must be [{}, {}, {}]: got {}".format(N, p.batch_size, p.n_classes, tuple(t.shape)))
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _evaluate_local(self, number_samples, noise, minibatch, seed, offset, want_noise, want_indices):
        p, N, dev = self.program, int(number_samples), self.device
        if offset is None:
            offset = self.iteration
            self.iteration += 1
        noise_o = torch.empty((N, p.batch_size, p.n_classes), device=dev) if want_noise else None
        idx_o = torch.empty(p.batch_size, device=dev, dtype=torch.int32) if want_indices else None
        noise_t, idx_t = self._local_noise(noise, N), self._indices_tensor(minibatch)
        args = self._local_args(N, seed, offset)
        ptr = lambda t: t.data_ptr() if t is not None else None
        args.noise_dev, args.noise_out_dev, args.indices_dev, args.indices_out_dev = ptr(noise_t), ptr(noise_o), ptr(idx_t), ptr(idx_o)
        native.check(self.lib.bsvi_dense_local_fwd_bwd(self.handle, C.byref(args)))
        self.grads_valid = True
        res = dict(loss=self.out[2], finite=self.out[3], nonfinite_count=self.out[1],
                   grads=self.out[OUT_HEADER:OUT_HEADER + p.n_params], n_local=N, sample_base=0)
        if want_noise:
            res["noise"] = noise_o
        if want_indices:
            res["indices"] = idx_o
        return res

    def _train_local(self, K, N, cfg, noise_seq, minibatch_seq, seed, pretraining_iterations):
        """one bsvi_dense_local_fwd_bwd and one bsvi_optimizer_step per iteration, both on the stream: the finite flag of the out block
        skips the step on the device and nothing synchronises inside the loop"""
        from brancher_amd import engine
        p, dev = self.program, self.device
        loss_curve, finite, state = engine.training_buffers(K, p.n_params, dev)
        offset0 = self.iteration
        self.iteration += K
        # one struct for the run: an iteration changes its offset, its slots of the curves and, when handed in, its noise and minibatch
        args = self._local_args(N, seed, offset0)
        call, step, handle, a_ref, cfg_ref = self.lib.bsvi_dense_local_fwd_bwd, self.lib.bsvi_optimizer_step, self.handle, C.byref(args), C.byref(cfg)
        params, out, st, stream = self.params.data_ptr(), self.out.data_ptr(), state.data_ptr(), args.stream
        masks = self.mask_first.data_ptr(), self.mask_all.data_ptr()
        loss0, finite0 = loss_curve.data_ptr(), finite.data_ptr()
        for it in range(K):
            if noise_seq is not None:
                nz = self._local_noise(noise_seq[it], N)
                args.noise_dev = nz.data_ptr()
            if minibatch_seq is not None:
                mb = self._indices_tensor(minibatch_seq[it])
                args.indices_dev = mb.data_ptr()
            args.offset, args.loss_slot_dev, args.finite_slot_dev = offset0 + it, loss0 + 4 * it, finite0 + 4 * it
            rc = call(handle, a_ref) or step(cfg_ref, params, out, st, masks[it > pretraining_iterations], p.n_params, stream)
            if rc:
                native.check(rc)
        self.grads_valid = True
        self.last_mode = "local"
        return loss_curve[:K], finite[:K]

    def _predict_rows(self, x):
        """the caller's rows as a contiguous f32 device tensor [M, P]: from [M, P], [M, P, 1] or the reference's [1, M, P, 1]"""
        a = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        if a.ndim == 4 and a.shape[0] == 1:
            a = a[0]
        if a.ndim == 3 and a.shape[-1] == 1:
            a = a[..., 0]
        P = self.program.n_features
        if a.ndim != 2:
            raise ValueError("predict takes rows as [M, {P}], [M, {P}, 1] or [1, M, {P}, 1]: got shape {}".format(
                tuple(x.shape) if hasattr(x, "shape") else np.shape(x), P=P))
        if a.shape[1] != P:
            raise ValueError("the rows have {} features, the model was built on {}".format(a.shape[1], P))
        if a.shape[0] < 1:
            raise ValueError("predict needs at least one row")
        return a.to(device=self.device, dtype=torch.float32).contiguous()

    def _predict(self, rows, n_sets, sets_per_split, **how):
        key = (n_sets, int(rows.shape[0]), int(sets_per_split or 0))
        ws = self.__dict__.get("_predict_ws")       # (one workspace kept: the shape of the last call)
        res, ws = native.dense_predict(self.handle, rows, n_sets, self.program.n_classes, sets_per_split=key[2],
                                       workspace=ws[1] if ws is not None and ws[0] == key else None, **how)
        self._predict_ws = (key, ws)
        res["n_rows"] = key[1]
        return res

    def predict(self, x, number_samples, seed=None, offset=None, noise=None, want_outputs=False, want_draws=False, want_noise=False,
                sample_base=0, sets_per_split=None):
        """Posterior predictive on rows the caller hands in (bsvi_dense_predict, csrc/dense_predict.inc), as `CompiledBnn.predict`:
        `number_samples` weight sets from the CURRENT posterior — the draw of a training launch at the same (seed, offset, sample_base),
        or `noise` ([C P, N], or named as the oracle takes it); a point estimate gives its value N times — against every row of `x`.
        Device tensors: "probs" [N, M, C] (softmax probabilities | the sigmoid of the logit), "mean" [M, C] (their mean over the sets,
        fixed order) and on request "outputs" [N, M, C] (logits), "draws" [N, M, C] (one draw of the likelihood per set and row:
        one-hot | 0 / 1) and "noise" [C P, N] (the eps drawn).  offset=None draws from the sampling range (1 << 62) + tick, as the
        samplers of the engine do; `self.iteration`, `self.out` and the gradients are left alone.  Not sharded: every rank computes all
        N sets.  sets_per_split (default: chosen from the chip) is the number of sets a workgroup walks; it moves the order of the
        mean's sum between different values of itself only."""
        p, N = self.program, int(number_samples)
        if N < 1:
            raise ValueError("number_samples must be at least 1")
        rows = self._predict_rows(x)
        if p.n_classes > 16:
            raise ValueError("predict samples weight sets of at most 16 classes: this handle of {} serves predict_particles".format(p.n_classes))
        if noise is not None and not isinstance(noise, dict) and tuple(noise.shape) != (p.n_noise, N):
            raise ValueError("noise must be [{}, {}]: got {}".format(p.n_noise, N, tuple(noise.shape)))
        noise_t = self._noise_tensor(noise, N, 0, N)
        if noise_t is not None:
            if tuple(noise_t.shape) != (p.n_noise, N):
                raise ValueError("noise must be [{}, {}]: got {}".format(p.n_noise, N, tuple(noise_t.shape)))
            noise_t = noise_t.to(device=self.device, dtype=torch.float32).contiguous()
        if offset is None:
            _engine._sample_tick[0] += 1
            offset = (1 << 62) + _engine._sample_tick[0]
        if not isinstance(seed, int) or seed is True:
            seed = _engine.shared_seed(seed, self.device)
        res = self._predict(rows, N, sets_per_split, params=self.params, noise=noise_t, seed=int(seed), offset=int(offset),
                            sample_base=int(sample_base), want_outputs=want_outputs, want_draws=want_draws, want_noise=want_noise)
        res.update(seed=int(seed), offset=int(offset))
        return res

    def predict_particles(self, table, x, dim=None, seed=None, offset=None, want_outputs=False, want_draws=False, sample_base=0,
                          sets_per_split=None):
        """The predictive of an ensemble of point estimates: row n of `table` [N, ld] (f32 on the device, contiguous; the layout of
        `native.dense_particles_fwd_bwd`, value r = c P + p, `dim` = C P values of a row, the rest padding) is weight set n, read in
        place.  The result of `predict` without "noise"; "mean" is the ensemble's predictive.  (seed, offset) only feed the draws."""
        p = self.program
        R = p.n_classes * p.n_features
        if dim is not None and int(dim) != R:
            raise ValueError("predict_particles: dim is {}, a weight set of this model has {} x {} = {} values".format(dim, p.n_classes, p.n_features, R))
        if not torch.is_tensor(table) or table.ndim != 2 or table.shape[0] < 1:
            raise ValueError("predict_particles: the table is a two-dimensional tensor [N, ld] of at least one row")
        if table.shape[1] < R:
            raise ValueError("predict_particles: the table has {} columns, a weight set of this model has {} x {} = {} values".format(
                table.shape[1], p.n_classes, p.n_features, R))
        rows = self._predict_rows(x)
        if offset is None:
            _engine._sample_tick[0] += 1
            offset = (1 << 62) + _engine._sample_tick[0]
        if not isinstance(seed, int) or seed is True:
            seed = _engine.shared_seed(seed, self.device) if want_draws else 0
        res = self._predict(rows, int(table.shape[0]), sets_per_split, table=table, seed=int(seed), offset=int(offset),
                            sample_base=int(sample_base), want_outputs=want_outputs, want_draws=want_draws)
        res.update(seed=int(seed), offset=int(offset))
        return res

    def evaluate_weighted(self, number_samples, f_weight, q_weight, seed, offset, noise=None, minibatch=None):
        """The second pass of a user-defined gradient estimator (`engine.custom_estimator_loss`), as
        `CompiledELBO.evaluate_weighted`: the draw and the minibatch of (seed, offset) again, and
        -(sum_n a_n grad f_n + b_n grad log q_n) in the output block (bsvi_dense_args::f_weight_dev / q_weight_dev; the
        model must have been created with the BlackBox estimator)."""
        from brancher_amd import engine
        if self._local():
            raise ValueError("evaluate_weighted: the 'local' estimator serves no caller-weighted gradients (a user-defined estimator "
                             "needs per-sample f and log q of the weights, which it never draws)")
        rank, world = engine.dist_info()
        base, n_local = engine.shard(number_samples, rank, world)
        a = f_weight.reshape(-1)[base:base + n_local].contiguous().float()
        b = q_weight.reshape(-1)[base:base + n_local].contiguous().float()
        noise_t = self._noise_tensor(noise, number_samples, base, n_local)
        idx_t = self._indices_tensor(minibatch)
        args = self._args(n_local, number_samples, base, noise_t, idx_t, seed, int(offset), f_weight=a, q_weight=b)
        native.check(self.lib.bsvi_dense_fwd_bwd(self.handle, C.byref(args)))
        engine.allreduce_sums(self.out)
        engine.check_exchange(self.device, self.params)
        native.check(self.lib.bsvi_dense_finalize(self.handle, C.c_void_p(self.out.data_ptr()), 1, self._stream()))
        self.grads_valid = True
        return self.out[OUT_HEADER:OUT_HEADER + self.program.n_params]

    def named_grads(self):
        g = self.out[OUT_HEADER:].detach().cpu().numpy()
        return {par.name: g[off:off + size].reshape(par.shape).copy() for par, off, size, _ in self.program.parameters}

    def named_params(self):
        t = self.params.detach().cpu().numpy()
        return {par.name: t[off:off + size].reshape(par.shape).copy() for par, off, size, _ in self.program.parameters}

    def train(self, number_iterations, number_samples, optimizer="Adam", noise_seq=None, minibatch_seq=None, seed=None,
              pretraining_iterations=0, allow_persistent=True, _force_sharded_path=False, **opt_params):
        from brancher_amd import engine
        cfg = native.make_opt_cfg(optimizer, **opt_params)
        if self._local():
            return self._train_local(int(number_iterations), int(number_samples), cfg, noise_seq, minibatch_seq, seed, pretraining_iterations)
        rank, world = engine.dist_info()
        base, n_local = engine.shard(number_samples, rank, world)
        if n_local == 0:
            raise ValueError("number_samples={} is smaller than the number of GPUs {}".format(number_samples, world))
        dev, p = self.device, self.program
        K = int(number_iterations)
        engine.broadcast_from_rank0(self.params)      # ranks step their own copies: they must start from the same values
        loss_curve, finite, state = engine.training_buffers(K, p.n_params, dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        offset0 = self.iteration
        self.iteration += K
        self.grads_valid = True
        for it in range(K):
            nz = None if noise_seq is None else self._noise_tensor(noise_seq[it], number_samples, base, n_local)
            mb = None if minibatch_seq is None else self._indices_tensor(minibatch_seq[it])
            args = self._args(n_local, number_samples, base, nz, mb, seed, offset0 + it)
            mask = self.mask_all if it > pretraining_iterations else self.mask_first
            if world == 1 and not _force_sharded_path:
                native.check(self.lib.bsvi_dense_step(self.handle, C.byref(args), C.byref(cfg), ptr(self.params), ptr(state),
                                                      ptr(mask), C.c_void_p(loss_curve.data_ptr() + 4 * it),
                                                      C.c_void_p(finite.data_ptr() + 4 * it)))
            else:
                native.check(self.lib.bsvi_dense_fwd_bwd(self.handle, C.byref(args)))
                engine.allreduce_sums(self.out)
                native.check(self.lib.bsvi_finalize_step(
                    C.byref(cfg), ptr(self.params), ptr(self.out), ptr(state), ptr(mask), p.n_params, number_samples,
                    C.c_void_p(loss_curve.data_ptr() + 4 * it), C.c_void_p(finite.data_ptr() + 4 * it), self._stream()))
        self.last_mode = "stepwise" if world == 1 else "stepwise+allreduce"
        if world > 1:
            engine.check_exchange(self.device, self.params)         # (an abandoned exchange poisoned a step: say so, loudly)
        return loss_curve[:K], finite[:K]


# every native call of a compiled program runs with its device current (engine._bound_to_device)
from brancher_amd import engine as _engine  # noqa: E402  (engine imports this module lazily)
CompiledDense = _engine._bound_to_device(CompiledDense)
