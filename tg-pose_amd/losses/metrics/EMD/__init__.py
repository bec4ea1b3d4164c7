from .emd_module import emdModule as emd

__all__ = ['emd']
