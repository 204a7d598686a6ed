from vstyler.clip import WanImageEncoder  # noqa: F401
