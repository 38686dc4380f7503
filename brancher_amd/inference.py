"""
Inference loop (`brancher/inference.py`).

``perform_inference`` keeps the reference signature and semantics (`inference.py:50-111`):
optimizers for the posterior and — because ``ReverseKL.learnable_model`` is True — for the
joint model; per iteration ``compute_loss`` -> finite check -> ``backward`` -> step of the
first optimizer, the others only when ``iteration > pretraining_iterations``; non-finite
losses warn and skip the step; the loss curve lands in ``diagnostics["loss curve"]``.

What changes is where it runs: the whole iteration is one or two kernel launches
(`engine.CompiledELBO.train`), the finite check and the optimizer step happen on the device
and nothing synchronises with the host inside the loop.  Deviations, on purpose:
  * one loss entry per iteration (the reference appends twice per good iteration,
    `inference.py:105,108`, which makes ``np.array(loss_list)`` raise under numpy >= 1.24);
  * "Numerical error, skipping sample" warnings are emitted after the loop (the flags are
    read back once), not inside it;
  * ``SteinVariationalGradientDescent.correct_gradient`` REPELS.  The reference (`inference.py:308-315`, "work in progress") adds
    ``(theta_i - theta_j) K_ij / bw`` to the gradient of particle i, and a descent step along it pulls the particles together:
    run on two one-dimensional particles at 0 and 1 with zero gradients (bandwidth 2 / log 2 = 2.885) it hands back -0.2914 for the
    particle at 0 and +0.2914 for the one at 1, so both step towards each other.  Here the term has the sign of Liu & Wang (2016),
    ``-(theta_i - theta_j) K_ij / bw``: +0.2914 and -0.2914 on the same input.
"""
import warnings
from abc import ABC, abstractmethod

import numpy as np

from brancher_amd import gradient_estimators
from brancher_amd import engine
from brancher_amd.optimizers import ProbabilisticOptimizer


def perform_inference(joint_model, number_iterations, number_samples=1,
                      optimizer='Adam', input_values={},
                      inference_method=None,
                      posterior_model=None, sampler_model=None,
                      pretraining_iterations=0,
                      **opt_params):
    if not inference_method:
        warnings.warn("The inference method was not specified, using the default reverse KL variational inference")
        inference_method = ReverseKL()
    if not posterior_model:
        posterior_model = joint_model.posterior_model
    if not sampler_model:
        sampler_model = getattr(inference_method, "sampler_model", None) or getattr(joint_model, "posterior_sampler", None)

    joint_model.update_observed_submodel()

    optimizers_list = []
    for model, wanted in ((posterior_model, True), (joint_model, inference_method.learnable_model),
                          (sampler_model, inference_method.learnable_sampler)):
        if wanted and model is not None:
            prob_opt = ProbabilisticOptimizer(model, optimizer, **opt_params)
            if prob_opt.optimizer:
                optimizers_list.append(prob_opt)

    inference_method.check_model_compatibility(joint_model, posterior_model, sampler_model)
    if hasattr(inference_method, "run") and not engine.is_custom_estimator(getattr(inference_method, "gradient_estimator", None)):
        # the methods of this module: the whole loop of `inference.py:95-108` runs on the device
        loss_curve, finite = inference_method.run(joint_model, posterior_model, sampler_model, number_iterations,
                                                  number_samples, optimizer, pretraining_iterations, **opt_params)
        losses = loss_curve.detach().cpu().numpy()
        flags = finite.detach().cpu().numpy()
    else:
        # a reference-style InferenceMethod (only compute_loss / correct_gradient, `inference.py:114-126`): the loop
        # stays here and every step goes through the same device kernels — compute_loss evaluates loss AND gradients in
        # one launch (engine.FusedLoss), ProbabilisticOptimizer.update() is the device optimizer step
        losses, flags = [], []
        for iteration in range(number_iterations):
            loss = inference_method.compute_loss(joint_model, posterior_model, sampler_model, number_samples)
            value = float(loss.detach().cpu())
            flags.append(1.0 if np.isfinite(value) else 0.0)
            if flags[-1]:
                for opt in optimizers_list:
                    opt.zero_grad()
                loss.backward()
                if hasattr(inference_method, "correct_gradient"):
                    inference_method.correct_gradient(joint_model, posterior_model, sampler_model, number_samples)
                for index, opt in enumerate(optimizers_list):
                    if index == 0 or iteration > pretraining_iterations:
                        opt.update()
            losses.append(value)
        losses, flags = np.array(losses, dtype=np.float32), np.array(flags)
    for _ in range(int((flags == 0).sum())):
        warnings.warn("Numerical error, skipping sample")
    joint_model.diagnostics.update({"loss curve": np.array(losses)})
    inference_method.post_process(joint_model)
    # torch modules used as links are trained IN PLACE by the reference (their nn.Parameters belong to the optimizers,
    # `optimizers.py:36-49`); here their tensors live in the engine's parameter buffer: written back
    posteriors = posterior_model if isinstance(posterior_model, (list, tuple)) else [posterior_model]     # (a list: particles)
    for link in engine.module_links_of(joint_model, *posteriors):
        link.sync_to_module()


class InferenceMethod(ABC):
    # `inference.py:114-126`

    @abstractmethod
    def check_model_compatibility(self, joint_model, posterior_model, sampler_model):
        pass

    @abstractmethod
    def compute_loss(self, joint_model, posterior_model, sampler_model, number_samples, input_values):
        pass

    @abstractmethod
    def post_process(self, joint_model):
        pass


class ReverseKL(InferenceMethod):
    # `inference.py:129-151`

    def __init__(self, gradient_estimator=gradient_estimators.PathwiseDerivativeEstimator):
        self.learnable_model = True
        self.needs_sampler = False
        self.learnable_sampler = False
        self.gradient_estimator = gradient_estimator

    def check_model_compatibility(self, joint_model, posterior_model, sampler_model):
        pass

    def compute_loss(self, joint_model, posterior_model, sampler_model, number_samples, input_values={}):
        return -joint_model.estimate_log_model_evidence(number_samples=number_samples,
                                                        method="ELBO", input_values=input_values,
                                                        for_gradient=True, posterior_model=posterior_model,
                                                        gradient_estimator=self.gradient_estimator)

    def correct_gradient(self, joint_model, posterior_model, sampler_model, number_samples, input_values={}):
        pass

    def post_process(self, joint_model):
        pass

    def run(self, joint_model, posterior_model, sampler_model, number_iterations, number_samples, optimizer,
            pretraining_iterations, **opt_params):
        """the loop of `inference.py:95-108`, executed by the engine"""
        compiled = engine.compile_model(joint_model, posterior_model, self.gradient_estimator)
        extra = {}
        if getattr(compiled, "prefers_stepwise", None) and compiled.prefers_stepwise(number_samples):
            extra["allow_persistent"] = False
        if getattr(compiled, "_minibatches", None):
            # observations that are minibatches of a dataset: the rows are drawn and gathered inside the training launch
            # (CompiledELBO.train, minibatch_loop; BSVI_MINIBATCH_LOOP=0 switches it off)
            extra["minibatch_loop"] = True
        self.last_compiled = compiled       # (what served the last run: its `last_mode` says how)
        return compiled.train(number_iterations, number_samples, optimizer,
                              pretraining_iterations=pretraining_iterations, **extra, **opt_params)


class MAP(ReverseKL):
    """Maximum a posteriori point estimates, `inference.py:251-275`: the "posterior" is a model of learnable
    RootVariables carrying the latents' names; the loss is -log p(theta, data).  On this engine that is the ELBO
    program of a posterior without random variables — nothing to sample, no entropy — evaluated on one sample
    (the reference also ignores number_samples here)."""

    def __init__(self):
        super().__init__(gradient_estimator=gradient_estimators.PathwiseDerivativeEstimator)
        self.learnable_model = False
        self.needs_sampler = False
        self.learnable_sampler = False

    def check_model_compatibility(self, joint_model, posterior_model, sampler_model):
        from brancher_amd.variables import RootVariable
        assert all([isinstance(var, RootVariable) for var in posterior_model.flatten()])

    def compute_loss(self, joint_model, posterior_model, sampler_model, number_samples, input_values={}):
        return super().compute_loss(joint_model, posterior_model, sampler_model, 1, input_values)

    def run(self, joint_model, posterior_model, sampler_model, number_iterations, number_samples, optimizer,
            pretraining_iterations, **opt_params):
        return super().run(joint_model, posterior_model, sampler_model, number_iterations, 1, optimizer,
                           pretraining_iterations, **opt_params)


class _ParticleLoss:
    """the sum of the particles' losses with the protocol the loop of `perform_inference` expects: ``backward()`` marks the gradient
    block of every particle's compiled program (each evaluation wrote its own) as the gradient of this value"""

    def __init__(self, losses):
        import torch
        self.losses = losses
        self.tensor = torch.stack([loss.tensor for loss in losses]).sum()

    def detach(self):
        return self.tensor.detach()

    def backward(self):
        for loss in self.losses:
            loss.backward()


class SteinVariationalGradientDescent(InferenceMethod):
    """Stein variational gradient descent (Liu & Wang 2016; `inference.py:277-327`): the posterior is a LIST of particles, each a model of
    learnable RootVariables named like the latents — what `MAP` takes, N times.  ``compute_loss`` is the sum of the particles' MAP losses
    (one compiled program and one launch per particle, loss and gradient together); ``correct_gradient`` couples the gradients on the
    device (`bsvi_svgd_direction`, csrc/svgd_kernel.hip: RBF kernel, the reference's median bandwidth unless ``bandwidth`` fixes it) and
    writes them back into the particles' gradient blocks, which ``ProbabilisticOptimizer.update()`` then steps with any optimizer.
    ``bandwidth`` holds the last bandwidth used once a run has ended.  The repulsion has the sign of the paper, not the reference's (the
    module docstring)."""
    MIN_PARTICLES, MAX_PARTICLES = 2, 256

    def __init__(self, bandwidth=None, batched=False):
        """``batched=True``: all particles of a Bayesian neural network, or of a logistic regression (the dense-link path), in one pass
        (`_run_batched`); a model the scalar path serves is refused, not served particle by particle."""
        self.batched = bool(batched)
        if self.batched:
            self.run = self._run_batched      # (an attribute of the instance: `perform_inference` hands the loop to a method with `run`)
        self._program = None
        self.learnable_model = False
        self.needs_sampler = False
        self.learnable_sampler = False
        if bandwidth is not None and not (np.isfinite(bandwidth) and bandwidth > 0):
            raise ValueError("bandwidth is None (the median rule) or a positive number")
        self.fixed_bandwidth = bandwidth
        self.bandwidth = bandwidth
        self._map = MAP()
        self._plan = None

    @staticmethod
    def _roots(particle):
        """the particle's variables in the one order every particle is laid out in: by name"""
        return sorted(particle.flatten(), key=lambda var: var.name)

    def check_model_compatibility(self, joint_model, posterior_model, sampler_model):
        from brancher_amd.variables import ProbabilisticModel, RootVariable
        if not isinstance(posterior_model, (list, tuple)) or not all(isinstance(p, ProbabilisticModel) for p in posterior_model):
            raise ValueError("SteinVariationalGradientDescent: posterior_model is a list of particles, each a ProbabilisticModel of learnable RootVariables")
        if not self.MIN_PARTICLES <= len(posterior_model) <= self.MAX_PARTICLES:
            raise ValueError("SteinVariationalGradientDescent: {} particles, the method takes {} .. {}".format(
                len(posterior_model), self.MIN_PARTICLES, self.MAX_PARTICLES))
        first = None
        for index, particle in enumerate(posterior_model):
            members = particle.flatten()
            # (a random variable first: its constants are roots that are not learnable, and it is the random variable that is to be named)
            for var in [v for v in members if not isinstance(v, RootVariable)] + [v for v in members if not getattr(v, "learnable", True)]:
                raise ValueError("SteinVariationalGradientDescent: particle {}: variable {!r} is a {}, a particle holds learnable "
                                 "RootVariables only".format(index, var.name, type(var).__name__ if not isinstance(var, RootVariable)
                                                             else "RootVariable that is not learnable"))
            layout = [(var.name, tuple(var.parameter.shape)) for var in self._roots(particle)]
            if first is None:
                first = layout
            names, names0 = [n for n, _ in layout], [n for n, _ in first]
            if names != names0:
                odd = sorted(set(names) ^ set(names0)) or names
                raise ValueError("SteinVariationalGradientDescent: particle {}: variable {!r} is not in every particle (particle 0 holds {})".format(
                    index, odd[0], ", ".join(names0)))
            for (name, shape), (_, shape0) in zip(layout, first):
                if shape != shape0:
                    raise ValueError("SteinVariationalGradientDescent: particle {}: variable {!r} has shape {}, particle 0 has {}".format(
                        index, name, shape, shape0))
        if self.batched and joint_model is not None:
            self._program = self._batched_program(joint_model, posterior_model)

    @staticmethod
    def _batched_program(joint_model, particles):
        """the lowered program all particles share (lowered with particle 0, no device work; `engine.compile_model` asks the paths in
        this order): a `dense.DenseProgram` (logistic regression: `bsvi_dense_particles_fwd_bwd`) or a Bayesian neural network's
        (`bsvi_bnn_particles_fwd_bwd`) — or the refusal: a model the scalar path serves is named with its path, and what the two calls
        do not serve with the feature (`dense.check_particles`, `bnn.check_particles`)"""
        from brancher_amd import bnn, dense, lowering
        what = "SteinVariationalGradientDescent(batched=True): "
        try:
            lowering.lower(joint_model, particles[0], "pathwise")
        except lowering.LoweringError:
            pass
        else:
            raise ValueError(what + "the model is served by the {}; the particles of a Bayesian neural network alone are evaluated in one "
                                    "pass (the BNN path, CompiledBnn): use batched=False".format("scalar path (CompiledELBO)"))
        try:      # a logistic regression (the dense-link path): its particles go through one fused kernel (csrc/dense_particles.inc)
            program = dense.lower_dense(joint_model, particles[0], "pathwise")
        except lowering.LoweringError:
            pass
        else:
            dense.check_particles(program, len(particles))
            return program
        try:
            program = bnn.lower_bnn(joint_model, particles[0], "pathwise")
        except lowering.LoweringError as err:
            raise ValueError(what + "the model is not a Bayesian neural network the BNN path serves ({})".format(err)) from None
        bnn.check_particles(program, len(particles))
        return program

    def _build_batched_plan(self, joint_model, particles):
        """once per list of particles: a CompiledBnn (its handle takes both products per particle) or CompiledDense of its own, with the
        call that evaluates all particles on it (`evaluate`: the two have one signature), whose parameter buffer and
        output block are extended by the [N][ld] table of the particles and the table of their gradients — the particles' STORE: every
        particle's parameters are bound to their row, in the latent vector's row order"""
        import torch
        from brancher_amd import bnn, dense, native
        from brancher_amd.native import OUT_HEADER
        if self._program is None:
            self._program = self._batched_program(joint_model, particles)
        program = self._program
        if isinstance(program, dense.DenseProgram):      # one tensor, the weight matrix, rows r = c P + p
            compiled, evaluate = dense.CompiledDense(joint_model, particles[0], "pathwise", program=program, particles=True), native.dense_particles_fwd_bwd
            tensors = [dict(name=program.latent_name, row0=0, size=program.n_classes * program.n_features)]
        else:
            compiled, evaluate = bnn.CompiledBnn(joint_model, particles[0], "pathwise", program=program), native.bnn_particles_fwd_bwd
            tensors = program.tensors
        n, dim = len(particles), sum(t["size"] for t in tensors)
        ld = (dim + 3) // 4 * 4
        # the table starts a multiple of four floats into both buffers (16-byte rows), behind the handle's own parameters and gradients
        # and one header of the optimizer step: its finite flag is out[base + 3]
        base = (max(program.n_params, 1) + 3) // 4 * 4 + OUT_HEADER
        table = np.zeros((n, ld), dtype=np.float32)
        by_name = {t["name"]: t for t in tensors}
        for row, particle in enumerate(particles):
            for var in particle.flatten():
                t = by_name[var.name]
                table[row, t["row0"]:t["row0"] + t["size"]] = var.parameter.numpy().reshape(-1)
        dev = compiled.device
        params = torch.zeros(base + n * ld, device=dev)
        params[:compiled.params.numel()] = compiled.params
        params[base:] = torch.from_numpy(table.reshape(-1)).to(dev)
        compiled.params, compiled.out = params, torch.zeros(OUT_HEADER + base + n * ld, device=dev)
        for row, particle in enumerate(particles):
            for var in particle.flatten():
                var.parameter.bind(compiled, base + row * ld + by_name[var.name]["row0"])
        mask = torch.zeros(n, ld, dtype=torch.uint8, device=dev)
        mask[:, :dim] = 1
        return dict(key=tuple(id(p) for p in particles), compiled=compiled, evaluate=evaluate, n=n, dim=dim, ld=ld, base=base, mask=mask.reshape(-1),
                    theta=params[base:].view(n, ld), grad=compiled.out[OUT_HEADER + base:].view(n, ld), flag=compiled.out[base + 3:base + 4],
                    loss=torch.zeros(n, device=dev), bandwidth=torch.zeros(1, device=dev), workspace=None, svgd_workspace=None)

    def _run_batched(self, joint_model, posterior_model, sampler_model, number_iterations, number_samples, optimizer,
                     pretraining_iterations, **opt_params):
        """the loop of `perform_inference` for ``batched=True``, three native calls an iteration whatever the number of particles:
        `bsvi_bnn_particles_fwd_bwd` or `bsvi_dense_particles_fwd_bwd` on the table that IS the particles' parameter store (loss and gradient of every particle; one
        minibatch, shared), `bsvi_svgd_direction` in place on the gradient table, one `bsvi_optimizer_step` over its N ld elements with
        per-element state.  No gather, no scatter, no launch per particle.  A non-finite loss skips the step, as the loop does."""
        import ctypes as C
        import torch
        from brancher_amd import native
        if self._plan is None or self._plan["key"] != tuple(id(p) for p in posterior_model) or "compiled" not in self._plan:
            self._plan = self._build_batched_plan(joint_model, posterior_model)
        plan = self._plan
        compiled, n, ld, base, theta, grad, loss = (plan[k] for k in ("compiled", "n", "ld", "base", "theta", "grad", "loss"))
        cfg = native.make_opt_cfg(optimizer, **opt_params)
        dev = compiled.device
        K = int(number_iterations)
        state = torch.zeros(4 * n * ld, device=dev)
        curve, finite = torch.zeros(K, device=dev), torch.zeros(K, device=dev)
        seed = int(compiled._seed(None))
        for it in range(K):
            plan["workspace"] = plan["evaluate"](compiled.handle, compiled.params, compiled.out, theta, grad, loss, seed=seed,
                                                 offset=compiled.iteration, workspace=plan["workspace"])
            compiled.iteration += 1
            curve[it] = loss.sum()
            finite[it] = plan["flag"][0] = torch.isfinite(curve[it]).float()
            if not bool(finite[it]):
                continue
            plan["svgd_workspace"] = native.svgd_direction(theta, grad, grad, dim=plan["dim"], bandwidth=self.fixed_bandwidth,
                                                           bandwidth_out=plan["bandwidth"], workspace=plan["svgd_workspace"])
            with torch.cuda.device(dev):
                native.check(compiled.lib.bsvi_optimizer_step(C.byref(cfg), C.c_void_p(compiled.params.data_ptr() + 4 * base),
                                                              C.c_void_p(compiled.out.data_ptr() + 4 * base), C.c_void_p(state.data_ptr()),
                                                              C.c_void_p(plan["mask"].data_ptr()), n * ld, compiled._stream()))
        compiled.grads_valid = True
        self.last_compiled = compiled
        return curve, finite

    def predict(self, joint_model, posterior_model, x, want_outputs=False, want_draws=False):
        """The predictive of the particle ensemble of a logistic regression (the dense-link path) on the rows `x`, all particles in one
        launch (`CompiledDense.predict_particles`, csrc/dense_predict.inc): "probs" [N, M, C] per particle, "mean" [M, C] the
        ensemble's predictive, on request "outputs" (logits) and "draws".  When this instance's batched plan holds these particles its
        table is read in place — no copy, no gather; otherwise an engine and the table of the particles' current values are built for
        the call.  Particles of a Bayesian neural network are refused here: `predict_network` serves them."""
        import torch
        from brancher_amd import dense, lowering
        self.check_model_compatibility(None, posterior_model, None)
        plan = self._plan
        if plan is not None and plan.get("key") == tuple(id(p) for p in posterior_model) and isinstance(plan.get("compiled"), dense.CompiledDense):
            compiled, table, dim = plan["compiled"], plan["theta"], plan["dim"]
        else:
            try:
                program = dense.lower_dense(joint_model, posterior_model[0], "pathwise")
            except lowering.LoweringError as err:
                raise ValueError("SteinVariationalGradientDescent.predict serves the particles of a logistic regression (the dense-link path); "
                                 "the predictive of the particles of a Bayesian neural network, or of another model, is not served "
                                 "({}); the particles of a Bayesian neural network: predict_network".format(err)) from None
            if not program.point_estimate:
                raise ValueError("SteinVariationalGradientDescent.predict: {} has a Normal posterior, a particle is a point estimate".format(program.latent_name))
            bound = [(par, par._store, par._offset) for par, _, _, _ in program.parameters]
            compiled = dense.CompiledDense(joint_model, posterior_model[0], "pathwise", program=program, particles=True)
            for par, store, offset in bound:                   # (the constructor bound them to itself)
                par.unbind() if store is None else par.bind(store, offset)
            dim = program.n_classes * program.n_features
            values = np.stack([next(v for v in particle.flatten() if v.name == program.latent_name).parameter.numpy().reshape(-1)
                               for particle in posterior_model]).astype(np.float32)
            table = torch.from_numpy(values).to(compiled.device)
        return compiled.predict_particles(table, x, dim=dim, want_outputs=want_outputs, want_draws=want_draws)

    def predict_network(self, joint_model, posterior_model, x, want_outputs=False, want_draws=False):
        """The predictive of the particle ensemble of a Bayesian neural network on the rows `x`, the whole chain of all particles in one
        fused kernel (`CompiledBnn.predict_particles`, csrc/bnn_ensemble.inc): "probs" [N, M, C] per particle, "mean" [M, C] the
        ensemble's predictive, "var" [M, C] where the likelihood has one, on request "outputs" (logits | loc) and "draws".  When this
        instance's batched plan holds these particles its table is read in place — no copy, no gather; otherwise an engine and the table
        of the particles' current values, in the tensors' row order, are built for the call and the parameters' bindings restored."""
        import torch
        from brancher_amd import bnn, lowering
        self.check_model_compatibility(None, posterior_model, None)
        plan = self._plan
        if plan is not None and plan.get("key") == tuple(id(p) for p in posterior_model) and isinstance(plan.get("compiled"), bnn.CompiledBnn):
            compiled, table, dim = plan["compiled"], plan["theta"], plan["dim"]
        else:
            try:
                program = bnn.lower_bnn(joint_model, posterior_model[0], "pathwise")
            except lowering.LoweringError as err:
                raise ValueError("SteinVariationalGradientDescent.predict_network serves the particles of a Bayesian neural network (the BNN "
                                 "path, CompiledBnn); this model is not one it lowers ({})".format(err)) from None
            bnn.check_particles(program, len(posterior_model))
            bound = [(par, par._store, par._offset) for par, _, _, _ in program.parameters]
            compiled = bnn.CompiledBnn(joint_model, posterior_model[0], "pathwise", program=program)
            for par, store, offset in bound:                   # (the constructor bound them to itself)
                par.unbind() if store is None else par.bind(store, offset)
            dim = program.n_rows
            values = np.zeros((len(posterior_model), dim), dtype=np.float32)
            by_name = {t["name"]: t for t in program.tensors}
            for row, particle in enumerate(posterior_model):
                for var in particle.flatten():
                    t = by_name[var.name]
                    values[row, t["row0"]:t["row0"] + t["size"]] = var.parameter.numpy().reshape(-1)
            table = torch.from_numpy(values).to(compiled.device)
        return compiled.predict_particles(table, x, dim=dim, want_outputs=want_outputs, want_draws=want_draws)

    def compute_loss(self, joint_model, posterior_model, sampler_model, number_samples, input_values={}):
        return _ParticleLoss([self._map.compute_loss(joint_model, particle, sampler_model, 1, input_values) for particle in posterior_model])

    def _build_plan(self, posterior_model):
        """once per list of particles: where every particle's values and gradients live (index tensors on the device, in the order of
        `_roots`) and the [N][D] buffers the kernels work on"""
        import torch
        from brancher_amd.native import OUT_HEADER
        rows = []
        for index, particle in enumerate(posterior_model):
            pars = [var.parameter for var in self._roots(particle)]
            stores = {id(par._store) for par in pars}
            if None in {par._store for par in pars} or len(stores) != 1:
                raise RuntimeError("particle {} is not part of one compiled model yet: evaluate the loss first".format(index))
            store = pars[0]._store
            idx = torch.from_numpy(np.concatenate([np.arange(par._offset, par._offset + par.size) for par in pars]).astype(np.int64)).to(store.device)
            rows.append((store, idx, idx + OUT_HEADER))
        device, dim = rows[0][0].device, rows[0][1].numel()
        if any(idx.numel() != dim or store.device != device for store, idx, _ in rows):
            raise RuntimeError("the particles differ in size or live on several devices")
        return dict(key=tuple(id(p) for p in posterior_model), rows=rows, workspace=None,
                    theta=torch.empty(len(rows), dim, device=device), grad=torch.empty(len(rows), dim, device=device),
                    bandwidth=torch.zeros(1, device=device))

    def correct_gradient(self, joint_model, posterior_model, sampler_model, number_samples, input_values={}):
        import torch
        from brancher_amd import native
        if self._plan is None or self._plan["key"] != tuple(id(p) for p in posterior_model):
            self._plan = self._build_plan(posterior_model)
        plan = self._plan
        theta, grad = plan["theta"], plan["grad"]
        for row, (store, idx, idx_out) in enumerate(plan["rows"]):
            if not getattr(store, "grads_valid", False):
                raise RuntimeError("no gradients: call compute_loss(...).backward() before correct_gradient()")
            torch.index_select(store.params, 0, idx, out=theta[row])
            torch.index_select(store.out, 0, idx_out, out=grad[row])
        plan["workspace"] = native.svgd_direction(theta, grad, grad, bandwidth=self.fixed_bandwidth, bandwidth_out=plan["bandwidth"],
                                                  workspace=plan["workspace"])
        for row, (store, idx, idx_out) in enumerate(plan["rows"]):
            store.out.index_copy_(0, idx_out, grad[row])

    def post_process(self, joint_model):
        if self._plan is not None:
            self.bandwidth = float(self._plan["bandwidth"].item())
