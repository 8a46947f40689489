"""What the Python front end answers before any device work, as a table of calls over the eleven public functions.

``no_device(error)`` makes every way to an engine raise ``error``; ``outcome(call)`` runs one call of the table under it and says
how it ended: ``[exception class, message]`` for a refusal, ``"DEVICE"`` when the call got as far as asking for an engine -- every
check had passed --, ``"RETURNED"`` when it came back without one.  tests/golden/make_golden_refusals.py records the table,
tests/test_frontend_cpu.py replays it.  Images are (1,3,16,18), kernels (1,1,3,5) where nothing else is said; every call takes
milliseconds and none reaches a GPU.  (The patch branch of PolyblurDeblurring moves a CPU tensor to the GPU before it asks for an
engine, so only its refusals are in the table.)"""
import contextlib
import sys

import numpy as np
import torch


class DeviceReached(Exception):
    pass


@contextlib.contextmanager
def no_device(error, library_too=True):
    """get_engine of every loaded polyblur_amd module that has one, Engine.__init__ and -- `library_too` -- _capi.load_library
    raise `error`"""
    import polyblur_amd  # noqa: F401
    from polyblur_amd import _capi as capi, engine

    def boom(*a, **k):
        raise error
    targets = [(mod, "get_engine") for name, mod in sorted(sys.modules.items())
               if name.startswith("polyblur_amd.") and hasattr(mod, "get_engine")]
    targets.append((engine.Engine, "__init__"))
    if library_too:
        targets.append((capi, "load_library"))
    saved = [(obj, name, getattr(obj, name)) for obj, name in targets]
    for obj, name in targets:
        setattr(obj, name, boom)
    try:
        yield
    finally:
        for obj, name, old in saved:
            setattr(obj, name, old)


def outcome(call):
    try:
        with no_device(DeviceReached(), library_too=False):       # (pb_fft_length_supported needs the library and no GPU)
            call()
    except DeviceReached:
        return "DEVICE"
    except Exception as e:
        return [type(e).__name__, str(e)]
    return "RETURNED"


IMAGE, KERNEL = (1, 3, 16, 18), (1, 1, 3, 5)
IMAGES = {                                                        # kind -> (maker, may require grad)
    "ndarray": (lambda: np.random.default_rng(0).random(IMAGE, dtype=np.float32), False),
    "ndarray-float64": (lambda: np.random.default_rng(0).random(IMAGE), False),
    "ndarray-rank3": (lambda: np.random.default_rng(0).random(IMAGE[1:], dtype=np.float32), False),
    "cpu": (lambda: torch.rand(IMAGE), True),
    "float16": (lambda: torch.rand(IMAGE).half(), True),
    "float64": (lambda: torch.rand(IMAGE).double(), True),
    "rank3": (lambda: torch.rand(IMAGE[1:]), True),
    "list": (lambda: [[0.5, 0.5], [0.5, 0.5]], False),
}
KERNELS = {
    "good": lambda: torch.rand(KERNEL), "ndarray": lambda: np.random.default_rng(1).random(KERNEL, dtype=np.float32),
    "even": lambda: torch.rand(1, 1, 4, 4), "one-wide": lambda: torch.rand(1, 1, 3, 1), "tall": lambda: torch.rand(1, 1, 5, 3),
    "above-49": lambda: torch.rand(1, 1, 51, 51), "too-large": lambda: torch.rand(1, 1, 21, 23), "tuple": lambda: (torch.rand(5), torch.rand(5)),
    "batch-2": lambda: torch.rand(2, 1, 3, 5), "channels-2": lambda: torch.rand(1, 2, 3, 5), "per-plane": lambda: torch.rand(1, 3, 3, 5),
    "rank3": lambda: torch.rand(1, 3, 5), "string": lambda: "gaussian", "empty": lambda: torch.rand(1, 1, 0, 5),
}


def image(kind, grad=False):
    x = IMAGES[kind][0]()
    return x.requires_grad_(True) if grad else x


def kernel(kind, grad=False):
    k = KERNELS[kind]()
    return k.requires_grad_(True) if grad else k


def planes(kind="cpu", grad=False):
    return (image(kind), image(kind, grad))


def table():
    """[(id, call)]: ids are the keys of tests/golden/frontend_refusals.json"""
    import polyblur_amd as pa
    rows = []

    def add(name, call):
        assert name not in dict(rows), name
        rows.append((name, call))

    # ---- the functions of a (B,C,H,W) image: every kind of image, with and without grad on it
    filters = {
        "convolve2d": lambda x, k, **kw: pa.convolve2d(x, k, **kw),
        "edgetaper": lambda x, k, **kw: pa.edgetaper(x, k, **kw),
        "inverse_filtering_rank3": lambda x, k, **kw: pa.inverse_filtering_rank3(x, k, 6, 1, **kw),
        "compute_polynomial": lambda x, k, **kw: pa.compute_polynomial(x, k, 6, 1, **kw),
        "inverse_filtering_nonsymmetric": lambda x, k, **kw: pa.inverse_filtering_nonsymmetric(x, k, 6, 1, **kw),
    }
    planar = dict(filters)
    planar["gaussian_blur_estimation"] = lambda x, k, **kw: pa.gaussian_blur_estimation(x, **kw)
    planar["fourier_gradients"] = lambda x, k, **kw: pa.fourier_gradients(x)
    planar["halo_masking"] = lambda x, k, **kw: pa.halo_masking(x, torch.rand(IMAGE), **kw)
    for fname, f in planar.items():
        for kind, (_, differentiable) in IMAGES.items():
            for grad in ((False, True) if differentiable else (False,)):
                add("%s/img=%s%s" % (fname, kind, "+grad" if grad else ""), lambda f=f, kind=kind, grad=grad: f(image(kind, grad), kernel("good")))
        add("%s/img=cpu+grad/no_grad" % fname, lambda f=f: _under_no_grad(lambda: f(image("cpu", True), kernel("good", True))))

    # ---- the kernel: shapes, kinds, grad on it, both boundary models
    for fname, f in filters.items():
        methods = (None,) if fname == "inverse_filtering_nonsymmetric" else ("fft", "direct")
        for kind in KERNELS:
            for method in methods:
                kw = {} if method is None else {"method": method}
                add("%s/kernel=%s/%s" % (fname, kind, method), lambda f=f, kind=kind, kw=kw: f(image("cpu"), kernel(kind), **kw))
        for kind in ("good", "even", "tall", "per-plane"):
            add("%s/kernel=%s+grad" % (fname, kind), lambda f=f, kind=kind: f(image("cpu"), kernel(kind, True)))
            add("%s/kernel=%s+grad/img=ndarray" % (fname, kind), lambda f=f, kind=kind: f(image("ndarray"), kernel(kind, True)))
            add("%s/kernel=%s+grad/img=cpu+grad" % (fname, kind), lambda f=f, kind=kind: f(image("cpu", True), kernel(kind, True)))
        add("%s/method=direct_separable" % fname, lambda f=f, fname=fname: f(image("cpu"), kernel("good"), **({} if fname == "inverse_filtering_nonsymmetric" else {"method": "direct_separable"})))
        if methods != (None,):
            add("%s/method=bogus" % fname, lambda f=f: f(image("cpu"), kernel("good"), method="bogus"))
    add("edgetaper/n_tapers=-1", lambda: pa.edgetaper(image("cpu"), kernel("good"), n_tapers=-1))
    add("edgetaper/n_tapers=1.5", lambda: pa.edgetaper(image("cpu"), kernel("good"), n_tapers=1.5))
    add("edgetaper/n_tapers=-1/img=rank3", lambda: pa.edgetaper(image("rank3"), kernel("good"), n_tapers=-1))
    for method in ("fft", "direct"):
        for grad in (False, True):
            add("compute_polynomial/not_symmetric/%s%s" % (method, "+grad" if grad else ""),
                lambda method=method, grad=grad: pa.compute_polynomial(image("cpu", grad), kernel("good"), 6, 1, method=method, not_symmetric=True))
    add("compute_polynomial/not_symmetric/side-8209", lambda: pa.compute_polynomial(torch.rand(1, 1, 16, 8209), kernel("good"), 6, 1, not_symmetric=True))
    add("inverse_filtering_nonsymmetric/side-8209", lambda: pa.inverse_filtering_nonsymmetric(torch.rand(1, 1, 16, 8205), kernel("good"), 6, 1))

    # ---- the chain's options: remove_halo with every grad_img, do_edgetaper, correlate
    for fname in ("inverse_filtering_rank3", "inverse_filtering_nonsymmetric"):
        f = filters[fname]
        grad_imgs = {"none": lambda: None, "good": planes, "short": lambda: (image("cpu"),), "not-a-pair": lambda: image("cpu"),
                     "other-shape": lambda: (torch.rand(1, 3, 16, 20), torch.rand(1, 3, 16, 20)), "ndarray": lambda: planes("ndarray"),
                     "float16": lambda: planes("float16"), "plane+grad": lambda: planes("cpu", True), "float16-plane+grad": lambda: planes("float16", True)}
        for gname, g in grad_imgs.items():
            for grad in (False, True):
                add("%s/remove_halo/grad_img=%s%s" % (fname, gname, "/img=cpu+grad" if grad else ""),
                    lambda f=f, g=g, grad=grad: f(image("cpu", grad), kernel("good"), remove_halo=True, grad_img=g()))
        add("%s/remove_halo/grad_img=good/img=ndarray" % fname, lambda f=f: f(image("ndarray"), kernel("good"), remove_halo=True, grad_img=planes()))
        add("%s/remove_halo/kernel=good+grad" % fname, lambda f=f: f(image("cpu"), kernel("good", True), remove_halo=True))
        add("%s/remove_halo/kernel=even/img=cpu+grad" % fname, lambda f=f: f(image("cpu", True), kernel("even"), remove_halo=True))
        add("%s/remove_halo=False/grad_img=plane+grad" % fname, lambda f=f: f(image("cpu"), kernel("good"), grad_img=planes("cpu", True)))
        add("%s/remove_halo=False/grad_img=short" % fname, lambda f=f: f(image("cpu"), kernel("good"), grad_img=(image("cpu"),)))
        add("%s/remove_halo/img=float16" % fname, lambda f=f: f(image("float16"), kernel("good"), remove_halo=True))
        add("%s/remove_halo/size-65537" % fname, lambda f=f: f(torch.rand(1, 1, 2, 65537), kernel("good"), remove_halo=True))
        for grad in (False, True):
            tag = "/img=cpu+grad" if grad else ""
            add("%s/do_edgetaper%s" % (fname, tag), lambda f=f, grad=grad: f(image("cpu", grad), kernel("good"), do_edgetaper=True))
            add("%s/do_edgetaper/kernel=tall%s" % (fname, tag), lambda f=f, grad=grad: f(image("cpu", grad), kernel("tall"), do_edgetaper=True))
            add("%s/correlate%s" % (fname, tag), lambda f=f, grad=grad: f(image("cpu", grad), kernel("good"), correlate=True))
            add("%s/do_edgetaper+remove_halo%s" % (fname, tag), lambda f=f, grad=grad: f(image("cpu", grad), kernel("good"), do_edgetaper=True, remove_halo=True))
    # (without grad these two are the one answer that differs from the recorded parent's: make_golden_refusals.py)
    for fname in ("inverse_filtering_rank3", "inverse_filtering_nonsymmetric"):
        add("%s/remove_halo/grad_img=mistyped" % fname, lambda f=filters[fname]: f(image("cpu"), kernel("good"), remove_halo=True, grad_img=([1.0], [2.0])))
        add("%s/remove_halo/grad_img=mistyped/img=cpu+grad" % fname, lambda f=filters[fname]: f(image("cpu", True), kernel("good"), remove_halo=True, grad_img=([1.0], [2.0])))

    # ---- halo masking and the spectral derivative
    add("halo_masking/imout=other-shape", lambda: pa.halo_masking(image("cpu"), torch.rand(1, 3, 16, 20)))
    add("halo_masking/imout=float16", lambda: pa.halo_masking(image("cpu"), image("float16")))
    add("halo_masking/imout=ndarray", lambda: pa.halo_masking(image("cpu"), image("ndarray")))
    add("halo_masking/imout=list", lambda: pa.halo_masking(image("cpu"), image("list")))
    add("halo_masking/imout+grad", lambda: pa.halo_masking(image("cpu"), image("cpu", True)))
    add("halo_masking/imout+grad/img=ndarray", lambda: pa.halo_masking(image("ndarray"), image("cpu", True)))
    add("halo_masking/grad_img=good", lambda: pa.halo_masking(image("cpu"), image("cpu"), planes()))
    add("halo_masking/grad_img=plane+grad", lambda: pa.halo_masking(image("cpu"), image("cpu"), planes("cpu", True)))
    add("halo_masking/grad_img=short", lambda: pa.halo_masking(image("cpu"), image("cpu"), (image("cpu"),)))
    add("halo_masking/grad_img=mistyped", lambda: pa.halo_masking(image("cpu"), image("cpu"), ([1.0], [2.0])))
    add("halo_masking/grad_img=other-shape", lambda: pa.halo_masking(image("cpu"), image("cpu"), (torch.rand(1, 3, 16, 20),) * 2))
    add("halo_masking/grad_img=short/img=rank3", lambda: pa.halo_masking(image("rank3"), image("cpu"), (image("cpu"),)))
    add("halo_masking/size-65537", lambda: pa.halo_masking(torch.rand(1, 1, 2, 65537), torch.rand(1, 1, 2, 65537)))
    add("halo_masking/size-65537+grad", lambda: pa.halo_masking(torch.rand(1, 1, 2, 65537, requires_grad=True), torch.rand(1, 1, 2, 65537)))
    add("fourier_gradients/size-65537", lambda: pa.fourier_gradients(torch.rand(1, 1, 65537, 2)))
    add("fourier_gradients/size-65537+grad", lambda: pa.fourier_gradients(torch.rand(1, 1, 65537, 2, requires_grad=True)))
    add("fourier_gradients/one-row", lambda: pa.fourier_gradients(torch.rand(1, 1, 1, 8)))

    # ---- the estimation's options
    est = pa.gaussian_blur_estimation
    for grad in (False, True):
        tag = "+grad" if grad else ""
        for k in (3, 24, 25, 27, 49, 50, 1, 2.5):
            add("gaussian_blur_estimation/ker_size=%r%s" % (k, tag), lambda k=k, grad=grad: est(image("cpu", grad), q=0, ker_size=k))
        add("gaussian_blur_estimation/ker_size=24/parameters%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, ker_size=24, return_2d_filters=False))
        add("gaussian_blur_estimation/parameters%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, return_2d_filters=False))
        for q in (0.0, 0.1, 0.5, -0.1):
            add("gaussian_blur_estimation/q=%r%s" % (q, tag), lambda q=q, grad=grad: est(image("cpu", grad), q=q))
        add("gaussian_blur_estimation/thetas=good%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, thetas=torch.linspace(0, 180, 7)))
        add("gaussian_blur_estimation/thetas=bad%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, thetas=torch.linspace(0, 180, 6)))
        add("gaussian_blur_estimation/interpolated_thetas=bad%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, interpolated_thetas=np.arange(30) * 5.0))
        add("gaussian_blur_estimation/n_angles=13%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, n_angles=13))
        add("gaussian_blur_estimation/multichannel/C=2%s" % tag, lambda grad=grad: est(torch.rand(1, 2, 16, 18, requires_grad=grad), q=0, multichannel=True))
        add("gaussian_blur_estimation/multichannel/C=3%s" % tag, lambda grad=grad: est(image("cpu", grad), q=0, multichannel=True))
        add("gaussian_blur_estimation/size-65537%s" % tag, lambda grad=grad: est(torch.rand(1, 1, 2, 65537, requires_grad=grad), q=0))
    add("gaussian_blur_estimation/float16+grad/q=0.1", lambda: est(image("float16", True), q=0.1))

    # ---- the blind call: the function, the module, the 8-bit function
    blind_images = {
        "ndarray-hwc": lambda: np.random.default_rng(0).random((16, 18, 3), dtype=np.float32), "ndarray-hw": lambda: np.random.default_rng(0).random((16, 18)),
        "ndarray-rank4": lambda: image("ndarray"), "cpu": lambda: image("cpu"), "float16": lambda: image("float16"), "float64": lambda: image("float64"),
        "rank3": lambda: image("rank3"), "uint8": lambda: (torch.rand(IMAGE) * 255).to(torch.uint8), "list": lambda: image("list"),
        "ndarray-uint8-hwc": lambda: np.zeros((16, 18, 3), np.uint8), "ndarray-uint8-hw": lambda: np.zeros((16, 18), np.uint8),
        "ndarray-uint8-rank4": lambda: np.zeros(IMAGE, np.uint8), "uint8-rank3": lambda: torch.zeros(IMAGE[1:], dtype=torch.uint8),
        "cpu+grad": lambda: image("cpu", True), "float16+grad": lambda: image("float16", True), "float64+grad": lambda: image("float64", True),
        "rank3+grad": lambda: image("rank3", True),
    }
    options = {
        "defaults": {}, "n_iter=0": dict(n_iter=0), "n_iter=-1": dict(n_iter=-1), "n_iter=1.5": dict(n_iter=1.5),
        "remove_halo": dict(remove_halo=True), "edgetaping": dict(edgetaping=True), "prefiltering": dict(prefiltering=True),
        "edgetaping+direct_separable": dict(edgetaping=True, method="direct_separable"), "direct_separable": dict(method="direct_separable"),
        "direct": dict(method="direct"), "method=bogus": dict(method="bogus"), "q=0.1": dict(q=0.1), "q=0.5": dict(q=0.5),
        "ker_size=24": dict(ker_size=24), "ker_size=31": dict(ker_size=31), "ker_size=50": dict(ker_size=50), "ker_size=1": dict(ker_size=1),
        "ker_size=24+direct_separable": dict(ker_size=24, method="direct_separable"), "ker_size=31+direct_separable": dict(ker_size=31, method="direct_separable"),
        "support=adaptive": dict(support="adaptive"), "support=bogus": dict(support="bogus"), "prefilter=bogus": dict(prefilter="bogus"),
        "temporaries=fp16": dict(temporaries="fp16"), "temporaries=bogus": dict(temporaries="bogus"), "return_info": dict(return_info=True),
        "multichannel_kernel": dict(multichannel_kernel=True), "n_angles=13": dict(n_angles=13), "n_interpolated_angles=65": dict(n_interpolated_angles=65),
        "device=1": dict(device=1), "remove_halo+edgetaping+q=0.1": dict(remove_halo=True, edgetaping=True, q=0.1),
        "return_info+temporaries=fp16+support=adaptive": dict(return_info=True, temporaries="fp16", support="adaptive"),
    }
    blind = {"polyblur_deblurring": pa.polyblur_deblurring, "PolyblurDeblurring": lambda x, **kw: pa.PolyblurDeblurring()(x, **kw),
             "polyblur_deblurring_uint8": pa.polyblur_deblurring_uint8}
    for fname, f in blind.items():
        for kind, make in blind_images.items():
            add("%s/img=%s" % (fname, kind), lambda f=f, make=make: f(make()))
        eight = fname == "polyblur_deblurring_uint8"
        for kind in (("uint8", "ndarray-uint8-hwc") if eight else ("cpu", "cpu+grad", "float16", "float16+grad", "ndarray-hwc")):
            for oname, kw in options.items():
                if (eight and "temporaries" in kw) or (fname == "PolyblurDeblurring" and oname == "device=1"):
                    continue                                   # (no such argument / a torch device there)
                add("%s/img=%s/%s" % (fname, kind, oname), lambda f=f, make=blind_images[kind], kw=kw: f(make(), **kw))
    add("polyblur_deblurring/C=2/multichannel_kernel", lambda: pa.polyblur_deblurring(torch.rand(1, 2, 16, 18), multichannel_kernel=True))
    add("polyblur_deblurring/size-65537", lambda: pa.polyblur_deblurring(torch.rand(1, 1, 2, 65537)))
    add("polyblur_deblurring/size-65537/ndarray", lambda: pa.polyblur_deblurring(np.zeros((2, 65537), np.float32)))
    add("polyblur_deblurring/size-65537+grad", lambda: pa.polyblur_deblurring(torch.rand(1, 1, 2, 65537, requires_grad=True)))
    add("polyblur_deblurring/cpu+grad/no_grad", lambda: _under_no_grad(lambda: pa.polyblur_deblurring(image("cpu", True))))
    add("PolyblurDeblurring/device=cpu", lambda: pa.PolyblurDeblurring()(image("cpu"), device="cpu"))

    def patches(x, module={}, **kw):
        return pa.PolyblurDeblurring(patch_decomposition=True, **dict(dict(patch_size=8), **module))(x, **kw)
    add("patches/img=cpu+grad", lambda: patches(image("cpu", True)))
    add("patches/img=cpu+grad/remove_halo", lambda: patches(image("cpu", True), remove_halo=True))
    add("patches/img=ndarray", lambda: patches(image("ndarray")))
    add("patches/img=rank3", lambda: patches(image("rank3")))
    add("patches/img=float64", lambda: patches(image("float64")))
    add("patches/return_info", lambda: patches(image("cpu"), return_info=True))
    add("patches/patch_size=1", lambda: patches(image("cpu"), module=dict(patch_size=1)))
    add("patches/patch_overlap=0.95", lambda: patches(image("cpu"), module=dict(patch_overlap=0.95)))
    add("patches/patch_size=400", lambda: patches(image("cpu"), module=dict(patch_size=400)))
    add("patches/device=cpu", lambda: patches(image("cpu"), device="cpu"))
    return rows


def _under_no_grad(call):
    with torch.no_grad():
        return call()
