"""differentiable_ransac_amd: see README.md.  Submodules are imported explicitly (`from differentiable_ransac_amd import ops`);
the names below are also reachable from the package itself, resolved on first use so that importing the package stays free."""
__all__ = ["BatchedRegistration", "BatchedHomography", "BatchedPnP"]


def __getattr__(name):
    if name in __all__:
        from . import ransac
        return getattr(ransac, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
