"""Deff as a differentiable torch op: the forward pass is a conjugate-gradient solve on the coefficient planes of the D map,
the backward pass the library's one-pass gradient (deff_sensitivity_D) -- no second solve, the problem is self-adjoint.
The concentration field as one: the same forward solve; the backward pass is one adjoint solve with the incoming gradient as
right-hand side (deff_solve_adjoint) and one pass over (x, lambda, D) (deff_field_vjp_D), for any loss on the field.
Both ops have a jvp for torch.autograd.forward_ad: Deff's is a sum over its gradient map, the field's one pass over (x, D, dD)
(deff_tangent_rhs_D) and one solve (deff_solve_tangent).  Deff is twice differentiable: under create_graph its backward hands
the gradient map out through a second Function whose backward is the Hessian-vector product -- the forward solve again, one
tangent solve and one pass over (x, dx, dD, D) (deff_sensitivity_hvp_D).  torch.func transforms are not supported (no
setup_context).  The field is twice differentiable too: under create_graph its backward is a Function (D, w) -> g whose own
backward gives S_w v -- the Hessian of w^T x(D) along v: the adjoint solve again, two tangent solves and one pass over
(x, lambda, dx, dlambda, v, D) (deff_field_vjp_hvp_D) -- for D and J v for w.

Volumes have the first order: effective_diffusivity_volume is Deff of a (nz, ny, nx) volume, its backward the one-pass gradient
(deff_volume_sensitivity_D), with the same jvp; it is once differentiable.

torch is imported inside the functions only: importing the package does not import it.  D makes a host round trip (plumbing;
the solve and the gradient run in the library's HIP kernels)."""
import numpy as np

from .solver import Solver, Volume

_FN = None
_GRAD_FN = None


def _tune(s, onchip):
    """The tuning keys every pass sets on its Solver: with `onchip` the solves on the coefficient planes iterate images of at
    most 16 384 cells on one compute unit each ("cg_onchip_planes" 1); without it the key is left as it is."""
    if onchip:
        s.set_tuning("cg_onchip_planes", 1)


def _grad_function():
    """The torch.autograd.Function that carries Deff's gradient map through a graph -- the second derivative of
    effective_diffusivity -- and the one its backward pass applies, the Hessian-vector product.  Created at first use."""
    global _GRAD_FN
    if _GRAD_FN is not None:
        return _GRAD_FN
    import torch

    class _DeffHessVec(torch.autograd.Function):
        """w -> H w per image, H the Hessian of deff_raw at D.  Linear in w and H is symmetric, so its own vjp is itself:
        torch.autograd.functional.hvp differentiates the backward pass with respect to the incoming gradient.  D is a
        constant here: third derivatives are not computed."""
        @staticmethod
        def forward(ctx, D, w, CL, CR, rtol, max_iter, solver, onchip):
            Dh = np.ascontiguousarray(D.detach().cpu().numpy(), dtype=np.float64)
            nimg = Dh.shape[0] if Dh.ndim == 3 else 1
            ny, nx = Dh.shape[-2:]
            wh = np.ascontiguousarray(w.detach().cpu().numpy(), dtype=np.float64)
            s = solver if solver is not None else Solver(nx, ny, nimg=nimg)
            try:
                # the forward pass's own calls: the same bits of x, whatever happened to the solver since
                s.assemble_from_D(Dh.reshape(nimg * ny, nx), CL, CR)
                s.init_linear(CL, CR)
                s.set_tuning("cg_planes", 1)
                _tune(s, onchip)
                _converged("effective_diffusivity (second order)", s.solve_cg(rtol=rtol, max_iter=max_iter), rtol, max_iter)
                try:
                    hv, _ = s.deff_hvp(Dh.reshape(nimg * ny, nx), wh.reshape(nimg * ny, nx), CL, CR, rtol=rtol, max_iter=max_iter)
                except RuntimeError as e:
                    raise RuntimeError(f"effective_diffusivity (second order): {e}") from None
            finally:
                if solver is None:
                    s.close()
            ctx.save_for_backward(D)
            ctx.deff_args = (CL, CR, rtol, max_iter, solver, onchip)
            return torch.from_numpy(np.ascontiguousarray(hv).reshape(Dh.shape)).to(w.device)

        @staticmethod
        def backward(ctx, u):
            (D,) = ctx.saved_tensors
            return None, _DeffHessVec.apply(D, u, *ctx.deff_args), None, None, None, None, None, None

    class _DeffGradient(torch.autograd.Function):
        @staticmethod
        def forward(ctx, D, g, CL, CR, rtol, max_iter, solver, onchip):
            # g(D) was computed by effective_diffusivity's forward pass: nothing is solved or copied here
            ctx.save_for_backward(D)
            ctx.deff_args = (CL, CR, rtol, max_iter, solver, onchip)
            return g.view_as(g)

        @staticmethod
        def backward(ctx, w):
            # H is symmetric: the vjp of the gradient map is the Hessian-vector product H w, per image
            (D,) = ctx.saved_tensors
            return _DeffHessVec.apply(D.detach(), w, *ctx.deff_args), None, None, None, None, None, None, None

    _GRAD_FN = _DeffGradient
    return _GRAD_FN


def _function():
    """The torch.autograd.Function, created at first use."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class _EffectiveDiffusivity(torch.autograd.Function):
        @staticmethod
        def forward(ctx, D, CL, CR, rtol, max_iter, solver, onchip):
            Dh = np.ascontiguousarray(D.detach().cpu().numpy(), dtype=np.float64)
            stack = Dh.ndim == 3
            nimg = Dh.shape[0] if stack else 1
            ny, nx = Dh.shape[-2:]
            s = solver if solver is not None else Solver(nx, ny, nimg=nimg)
            try:
                if (s.nx, s.ny, s.nimg) != (nx, ny, nimg):
                    raise ValueError(f"solver is {s.nimg} x ({s.ny}, {s.nx}), D is {tuple(Dh.shape)}")
                s.assemble_from_D(Dh.reshape(nimg * ny, nx), CL, CR)
                s.init_linear(CL, CR)
                s.set_tuning("cg_planes", 1)
                _tune(s, onchip)
                rs = s.solve_cg(rtol=rtol, max_iter=max_iter)
                rs = rs if isinstance(rs, list) else [rs]
                bad = [k for k, r in enumerate(rs) if not r.converged]
                if bad:
                    raise RuntimeError(f"effective_diffusivity: CG did not converge to rtol {rtol} for image(s) {bad} "
                                       f"(rel_residual {[rs[k].rel_residual for k in bad]}, max_iter {max_iter})")
                g, _ = s.sensitivity(Dh.reshape(nimg * ny, nx), CL, CR)
            finally:
                if solver is None:
                    s.close()
            deff = np.array([r.deff_raw for r in rs], dtype=np.float64)
            g = torch.from_numpy(np.ascontiguousarray(g).reshape(Dh.shape)).to(D.device)
            ctx.save_for_backward(g, D)
            ctx.save_for_forward(g)
            ctx.deff_args = (CL, CR, rtol, max_iter, solver, onchip)
            out = torch.from_numpy(deff).to(D.device)
            return out if stack else out[0]

        @staticmethod
        def backward(ctx, grad_out):
            g, D = ctx.saved_tensors
            if torch.is_grad_enabled() and D.requires_grad:
                # create_graph: the map as a function of D, whose backward is the Hessian-vector product
                g = _grad_function().apply(D, g, *ctx.deff_args)
            return grad_out[..., None, None] * g, None, None, None, None, None, None

        @staticmethod
        def jvp(ctx, tD, *_):
            # forward mode (torch.autograd.forward_ad): the map is the whole Jacobian, one row per image
            g = ctx.saved_tensors[0]
            return (g * tD).sum((-2, -1))

    _FN = _EffectiveDiffusivity
    return _FN


def effective_diffusivity(D, CL=0.0, CR=1.0, rtol=1e-12, max_iter=1_000_000, solver=None, onchip=False):
    """deff_raw of the diffusivity map D -- a float64 tensor (ny, nx), or (nimg, ny, nx) for a stack, on any device -- as a
    tensor on D's device, shape () or (nimg,), differentiable with respect to D.  Forward: deff_assemble_from_D, the linear
    guess, conjugate gradients on the coefficient planes to rtol (raises RuntimeError if they do not converge), then the
    gradient map of the converged field; backward: grad_out[..., None, None] * g.  `solver`: a Solver of the same shape to
    reuse (its system, field and the tuning key "cg_planes" are overwritten); otherwise one is created and closed.
    Twice differentiable: under create_graph=True the backward pass returns the same numbers with g as a function of D, and a
    backward pass through that (torch.autograd.functional.hvp, Newton-CG, a penalty on the gradient) gets H w, H the Hessian of
    deff_raw, per image: the system is assembled from D again, the linear guess taken and the forward pass's CG run again
    (the same bits of x), then Solver.deff_hvp -- one pass over (x, D, w), one tangent solve to rtol, one pass over
    (x, dx, w, D) -- on `solver` when one was passed (its system, field, tangent right-hand side map, tangent field, the
    Hessian-vector map and "cg_planes" are overwritten), otherwise on a Solver created and closed for that pass; RuntimeError
    if a solve does not converge.  H w is in turn differentiable with respect to w (by H again: functional.hvp's double
    backward needs it); D is a constant there, so third derivatives come out as zero, and a jvp of the gradient map and
    torch.func are not supported.  First-order use pays nothing for this: no extra solve or copy, the same bits.
    `onchip`: True sets the tuning key "cg_onchip_planes" to 1 on the Solver of every pass, first and second order, created
    here or passed (the key is overwritten, like "cg_planes", and stays set on a passed solver): images of at most 16 384
    cells (pitch x ny) iterate on one compute unit each (plan "cg_impl" 4), larger ones as without it.  The results agree with
    onchip=False to the solves' rtol, not bit for bit.  False (default) leaves the key alone: the same calls and bits as ever."""
    import torch
    if not isinstance(D, torch.Tensor) or D.dtype != torch.float64 or D.dim() not in (2, 3):
        raise TypeError("D must be a float64 tensor of shape (ny, nx) or (nimg, ny, nx)")
    return _function().apply(D, float(CL), float(CR), float(rtol), int(max_iter), solver, bool(onchip))


_VOLUME_FN = None


def _volume_function():
    """The torch.autograd.Function of effective_diffusivity_volume, created at first use."""
    global _VOLUME_FN
    if _VOLUME_FN is not None:
        return _VOLUME_FN
    import torch
    from torch.autograd.function import once_differentiable

    class _EffectiveDiffusivityVolume(torch.autograd.Function):
        @staticmethod
        def forward(ctx, D, CL, CR, rtol, max_iter, volume):
            Dh = np.ascontiguousarray(D.detach().cpu().numpy(), dtype=np.float64)
            nz, ny, nx = Dh.shape
            v = volume if volume is not None else Volume(nx, ny, nz)
            try:
                if (v.nx, v.ny, v.nz) != (nx, ny, nz):
                    raise ValueError(f"volume is ({v.nz}, {v.ny}, {v.nx}), D is {tuple(Dh.shape)}")
                v.assemble_from_D(Dh, CL, CR)
                v.init_linear(CL, CR)
                r = v.solve_cg(rtol=rtol, max_iter=max_iter)
                _converged("effective_diffusivity_volume", r, rtol, max_iter)
                g, _ = v.sensitivity(Dh, CL, CR)
            finally:
                if volume is None:
                    v.close()
            g = torch.from_numpy(g).to(D.device)
            ctx.save_for_backward(g)
            ctx.save_for_forward(g)
            return torch.tensor(r.deff_raw, dtype=torch.float64, device=D.device)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_out):
            (g,) = ctx.saved_tensors
            return grad_out * g, None, None, None, None, None

        @staticmethod
        def jvp(ctx, tD, *_):
            # forward mode (torch.autograd.forward_ad): the map is the whole Jacobian
            return (ctx.saved_tensors[0] * tD).sum()

    _VOLUME_FN = _EffectiveDiffusivityVolume
    return _VOLUME_FN


def effective_diffusivity_volume(D, CL=0.0, CR=1.0, rtol=1e-10, max_iter=1_000_000, volume=None):
    """deff_raw of the diffusivity volume D -- a float64 tensor (nz, ny, nx) on any device; a 3-D tensor given to
    effective_diffusivity is a stack of images and stays one -- as a 0-d tensor on D's device, differentiable with respect to
    D.  Forward: Volume.assemble_from_D, the linear guess, conjugate gradients to rtol (raises RuntimeError if they do not
    converge), then the gradient map of the converged field in one pass (deff_volume_sensitivity_D); backward: grad_out * g.
    Once differentiable: a backward pass under create_graph=True gives a gradient that cannot be differentiated again, and
    torch says so.  Under torch.autograd.forward_ad the tangent is (g * tD).sum().  `volume`: a Volume of the same shape to
    reuse (its system, field and gradient map are overwritten); otherwise one is created and closed.  D makes a host round
    trip."""
    import torch
    if not isinstance(D, torch.Tensor) or D.dtype != torch.float64 or D.dim() != 3:
        raise TypeError("D must be a float64 tensor of shape (nz, ny, nx)")
    return _volume_function().apply(D, float(CL), float(CR), float(rtol), int(max_iter), volume)


_FIELD_FN = None


def _converged(who, rs, rtol, max_iter):
    rs = rs if isinstance(rs, list) else [rs]
    bad = [k for k, r in enumerate(rs) if not r.converged]
    if bad:
        raise RuntimeError(f"{who}: CG did not converge to rtol {rtol} for image(s) {bad} "
                           f"(rel_residual {[rs[k].rel_residual for k in bad]}, max_iter {max_iter})")


_FIELD_GRAD_FN = None


def _field_grad_function():
    """The torch.autograd.Function (D, w) -> g = J^T w that carries the field adjoint's map through a graph -- the second
    derivative of concentration_field -- and the two its backward pass applies.  Created at first use."""
    global _FIELD_GRAD_FN
    if _FIELD_GRAD_FN is not None:
        return _FIELD_GRAD_FN
    import torch

    def on_solver(Dh, x, CL, CR, solver, onchip, fn):
        """fn(s, D2) on `solver`, or on a Solver created and closed here, with the system of Dh assembled and x as its field."""
        nimg = Dh.shape[0] if Dh.ndim == 3 else 1
        ny, nx = Dh.shape[-2:]
        s = solver if solver is not None else Solver(nx, ny, nimg=nimg)
        try:
            # whatever happened to the solver since the forward pass: its system and field are set again
            D2 = Dh.reshape(nimg * ny, nx)
            s.assemble_from_D(D2, CL, CR)
            s.set_field(x.reshape(nimg * ny, nx))
            _tune(s, onchip)
            return fn(s, D2)
        finally:
            if solver is None:
                s.close()

    def host(t, Dh):
        return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float64).reshape(-1, Dh.shape[-1])

    def tensor(a, Dh, like):
        return torch.from_numpy(np.ascontiguousarray(a).reshape(Dh.shape)).to(like.device)

    class _FieldHessVec(torch.autograd.Function):
        """v -> S_w v, S_w the Hessian of w^T x(D) with w fixed.  Linear in v and S_w is symmetric, so its own vjp is itself:
        torch.autograd.functional.hvp differentiates the backward pass with respect to the incoming gradient.  D and w are
        constants here: third derivatives and the w-derivative of S_w v are not computed."""
        @staticmethod
        def forward(ctx, v, Dh, x, w, CL, CR, rtol, max_iter, solver, onchip):
            def run(s, D2):
                _converged("concentration_field (second order, adjoint)",
                           s.solve_adjoint(w, rtol=rtol, max_iter=max_iter), rtol, max_iter)
                try:
                    return s.field_hvp(D2, host(v, Dh), CL, CR, rtol=rtol, max_iter=max_iter)[0]
                except RuntimeError as e:
                    raise RuntimeError(f"concentration_field (second order): {e}") from None
            ctx.deff_args = (Dh, x, w, CL, CR, rtol, max_iter, solver, onchip)
            return tensor(on_solver(Dh, x, CL, CR, solver, onchip, run), Dh, v)

        @staticmethod
        def backward(ctx, u):
            return (_FieldHessVec.apply(u, *ctx.deff_args),) + (None,) * 9

    class _FieldJvp(torch.autograd.Function):
        """v -> J v, J = dx/dD.  Linear in v; its vjp is J^T, the field adjoint's map with D held constant."""
        @staticmethod
        def forward(ctx, v, Dh, x, CL, CR, rtol, max_iter, solver, onchip):
            def run(s, D2):
                try:
                    return s.field_jvp(D2, host(v, Dh), CL, CR, rtol=rtol, max_iter=max_iter)
                except RuntimeError as e:
                    raise RuntimeError(f"concentration_field (second order): {e}") from None
            ctx.deff_args = (Dh, x, CL, CR, rtol, max_iter, solver, onchip)
            return tensor(on_solver(Dh, x, CL, CR, solver, onchip, run), Dh, v)

        @staticmethod
        def backward(ctx, u):
            Dh = ctx.deff_args[0]
            return (_FieldVjp.apply(tensor(Dh, Dh, u), u, *ctx.deff_args),) + (None,) * 8

    class _FieldVjp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, D, w, Dh, x, CL, CR, rtol, max_iter, solver, onchip):
            # concentration_field's first-order backward pass, call for call
            wh = host(w, Dh)

            def run(s, D2):
                _converged("concentration_field (adjoint)", s.solve_adjoint(wh, rtol=rtol, max_iter=max_iter), rtol, max_iter)
                return s.field_vjp(D2, CL, CR)[0]
            ctx.deff_args = (Dh, x, CL, CR, rtol, max_iter, solver, onchip)
            ctx.deff_w = wh
            return tensor(on_solver(Dh, x, CL, CR, solver, onchip, run), Dh, w)

        @staticmethod
        def backward(ctx, v):
            Dh, x, CL, CR, rtol, max_iter, solver, onchip = ctx.deff_args
            gD = gw = None
            if ctx.needs_input_grad[0]:
                gD = _FieldHessVec.apply(v, Dh, x, ctx.deff_w, CL, CR, rtol, max_iter, solver, onchip)
            if ctx.needs_input_grad[1]:
                gw = _FieldJvp.apply(v, *ctx.deff_args)
            return (gD, gw) + (None,) * 8

    _FIELD_GRAD_FN = _FieldVjp
    return _FIELD_GRAD_FN


def _field_function():
    """The torch.autograd.Function of concentration_field, created at first use."""
    global _FIELD_FN
    if _FIELD_FN is not None:
        return _FIELD_FN
    import torch

    class _ConcentrationField(torch.autograd.Function):
        @staticmethod
        def forward(ctx, D, CL, CR, rtol, max_iter, solver, onchip):
            Dh = np.ascontiguousarray(D.detach().cpu().numpy(), dtype=np.float64)
            nimg = Dh.shape[0] if Dh.ndim == 3 else 1
            ny, nx = Dh.shape[-2:]
            s = solver if solver is not None else Solver(nx, ny, nimg=nimg)
            try:
                if (s.nx, s.ny, s.nimg) != (nx, ny, nimg):
                    raise ValueError(f"solver is {s.nimg} x ({s.ny}, {s.nx}), D is {tuple(Dh.shape)}")
                s.assemble_from_D(Dh.reshape(nimg * ny, nx), CL, CR)
                s.init_linear(CL, CR)
                s.set_tuning("cg_planes", 1)
                _tune(s, onchip)
                _converged("concentration_field", s.solve_cg(rtol=rtol, max_iter=max_iter, fluxes=False), rtol, max_iter)
                x = s.get_field().reshape(Dh.shape)
            finally:
                if solver is None:
                    s.close()
            ctx.deff_args = (Dh, x, CL, CR, rtol, max_iter, solver, onchip)
            ctx.save_for_backward(D)
            return torch.from_numpy(x.copy()).to(D.device)

        @staticmethod
        def backward(ctx, grad_out):
            Dh, x, CL, CR, rtol, max_iter, solver, onchip = ctx.deff_args
            (D,) = ctx.saved_tensors
            if torch.is_grad_enabled() and (D.requires_grad or grad_out.requires_grad):
                # create_graph: the same calls inside a Function of (D, w), whose backward is the second order
                return (_field_grad_function().apply(D, grad_out, *ctx.deff_args),) + (None,) * 6
            nimg = Dh.shape[0] if Dh.ndim == 3 else 1
            ny, nx = Dh.shape[-2:]
            w = np.ascontiguousarray(grad_out.detach().cpu().numpy(), dtype=np.float64)
            s = solver if solver is not None else Solver(nx, ny, nimg=nimg)
            try:
                # whatever happened to the solver since the forward pass: its system and field are set again
                s.assemble_from_D(Dh.reshape(nimg * ny, nx), CL, CR)
                s.set_field(x.reshape(nimg * ny, nx))
                _tune(s, onchip)
                _converged("concentration_field (adjoint)",
                           s.solve_adjoint(w.reshape(nimg * ny, nx), rtol=rtol, max_iter=max_iter), rtol, max_iter)
                g, _ = s.field_vjp(Dh.reshape(nimg * ny, nx), CL, CR)
            finally:
                if solver is None:
                    s.close()
            g = torch.from_numpy(np.ascontiguousarray(g).reshape(Dh.shape)).to(grad_out.device)
            return g, None, None, None, None, None, None

        @staticmethod
        def jvp(ctx, tD, *_):
            # forward mode (torch.autograd.forward_ad): A dx = db - dA x along tD, one pass and one solve
            Dh, x, CL, CR, rtol, max_iter, solver, onchip = ctx.deff_args
            nimg = Dh.shape[0] if Dh.ndim == 3 else 1
            ny, nx = Dh.shape[-2:]
            d = np.ascontiguousarray(tD.detach().cpu().numpy(), dtype=np.float64)
            s = solver if solver is not None else Solver(nx, ny, nimg=nimg)
            try:
                # as in backward: the solver's system and field are set again
                s.assemble_from_D(Dh.reshape(nimg * ny, nx), CL, CR)
                s.set_field(x.reshape(nimg * ny, nx))
                _tune(s, onchip)
                s.tangent_rhs(Dh.reshape(nimg * ny, nx), d.reshape(nimg * ny, nx), CL, CR)
                _converged("concentration_field (tangent)", s.solve_tangent(rtol=rtol, max_iter=max_iter), rtol, max_iter)
                dx = s.get_tangent()
            finally:
                if solver is None:
                    s.close()
            return torch.from_numpy(dx.reshape(Dh.shape)).to(tD.device)

    _FIELD_FN = _ConcentrationField
    return _FIELD_FN


def concentration_field(D, CL=0.0, CR=1.0, rtol=1e-12, max_iter=1_000_000, solver=None, onchip=False):
    """The concentration field x of the diffusivity map D -- a float64 tensor (ny, nx), or (nimg, ny, nx) for a stack, on any
    device -- as a tensor of D's shape on D's device, differentiable with respect to D for ANY loss on x.  Forward, as
    effective_diffusivity: deff_assemble_from_D, the linear guess, conjugate gradients on the coefficient planes to rtol
    (RuntimeError if they do not converge).  Backward, with the incoming gradient w = dL/dx: the system is assembled from D
    again and the saved x set as its field -- on `solver` when one was passed, otherwise on a Solver created and closed for the
    backward pass --, then one adjoint solve A lambda = w to rtol (deff_solve_adjoint; RuntimeError if it does not converge)
    and one pass over (x, lambda, D) (deff_field_vjp_D) give dL/dD.  D and w make a host round trip.  `solver`: a Solver of the
    same shape to reuse (its system, field, adjoint field and the tuning key "cg_planes" are overwritten, in both passes).
    Under torch.autograd.forward_ad the tangent of x along D's tangent is computed the same way: system and field set again,
    then deff_tangent_rhs_D and deff_solve_tangent to rtol (RuntimeError if it does not converge).
    Twice differentiable: under create_graph=True the backward pass makes the same calls and returns the same numbers, as a
    function g(D, w) of D and the incoming gradient.  A backward pass through that with a cotangent v (functional.hvp,
    Newton-CG, a penalty on the gradient) gets, for D, S_w v -- S_w the Hessian of w^T x(D) with w fixed, the term that makes the
    Gauss-Newton product J^T L'' J into the Hessian: system and field set again, deff_solve_adjoint(w), then Solver.field_hvp
    (deff_tangent_rhs_D, deff_solve_tangent, deff_adjoint_tangent_rhs_D, deff_solve_adjoint_tangent, deff_field_vjp_hvp_D) --
    and, for w, J v (Solver.field_jvp); each on `solver` when one was passed (its system, field, adjoint field, both tangents'
    right-hand side maps, the tangent field, the adjoint's tangent and the second-order map are overwritten), otherwise on a
    Solver created and closed for that pass; RuntimeError if a solve does not converge.  S_w v and J v are in turn
    differentiable with respect to v (by S_w again, and by J^T: functional.hvp's double backward needs both); D and w are
    constants there, so third derivatives and the w-derivative of S_w v come out as None / zero, and a jvp of the gradient map and
    torch.func are not supported.  First-order use pays nothing for this: the same calls, the same bits, no graph.
    `onchip`: as in effective_diffusivity -- True sets "cg_onchip_planes" to 1 on the Solver of the forward pass, the backward
    pass, the jvp and every second-order pass (created or passed; the key is overwritten), so the forward solve and the
    adjoint and tangent solves iterate eligible images on one compute unit each; False (default) leaves the key alone."""
    import torch
    if not isinstance(D, torch.Tensor) or D.dtype != torch.float64 or D.dim() not in (2, 3):
        raise TypeError("D must be a float64 tensor of shape (ny, nx) or (nimg, ny, nx)")
    return _field_function().apply(D, float(CL), float(CR), float(rtol), int(max_iter), solver, bool(onchip))
