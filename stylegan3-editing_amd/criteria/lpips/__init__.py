from criteria.lpips.lpips import LPIPS  # noqa: F401
