"""differentiable_ransac_amd: see README.md.  Submodules are imported explicitly (`from differentiable_ransac_amd import ops`);
the names below are also reachable from the package itself, resolved on first use so that importing the package stays free."""
__all__ = ["BatchedRegistration"]


def __getattr__(name):
    if name == "BatchedRegistration":
        from .ransac import BatchedRegistration
        return BatchedRegistration
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
