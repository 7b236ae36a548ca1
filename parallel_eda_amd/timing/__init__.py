from .sta import STA, ConstrainedSTA

__all__ = ["STA", "ConstrainedSTA"]
