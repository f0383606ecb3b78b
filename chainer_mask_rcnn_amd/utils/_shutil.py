"""git_hash — the reference's chainer_mask_rcnn/utils/_shutil.py."""
import os
import subprocess


def git_hash(filename=None):
    """Abbreviated hash of the last commit of the git tree containing ``filename`` (the current
    directory when None), or None outside a git tree."""
    cwd = None if filename is None else os.path.dirname(os.path.abspath(filename))
    try:
        return subprocess.check_output(['git', 'log', '-1', '--format=%h'], cwd=cwd,
                                       stderr=subprocess.DEVNULL).decode().strip() or None
    except Exception:
        return None
