from .msg_norm import MessageNorm

__all__ = ['MessageNorm']
