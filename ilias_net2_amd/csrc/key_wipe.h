/*
 * key_wipe.h -- zeroing key material a launcher held on its stack (key
 * blocks, midstates, key schedules) once the launch has copied its arguments.
 * Host-safe: no HIP header, no device qualifier.
 */
#ifndef NET2_KEY_WIPE_H
#define NET2_KEY_WIPE_H

#include <stddef.h>
#include <stdint.h>

/* (volatile stores: not removed as dead ahead of the object's end of life) */
inline void key_wipe(void *p, size_t n)
{
	volatile uint8_t *z = (volatile uint8_t *)p;
	while (n-- > 0)
		*z++ = 0;
}

#endif /* NET2_KEY_WIPE_H */
